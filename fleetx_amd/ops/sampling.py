"""Fused top-k / top-p sampling (K18; csrc/kernels/sampling.hip).

One launch per decode step replaces softmax -> topk -> sort/cumsum/scatter ->
multinomial -> log_softmax/gather (reference ``single_model.py:907-988``).
The uniforms come from a torch generator so seeded generation is
reproducible; CPU tensors take the PyTorch reference path
(``generation.top_k_filter`` / ``top_p_filter`` + ``torch.multinomial``).

``coupled_sample`` is the coupled sampler: a Gumbel race over the same kept
set with noise that depends only on ``(seed, token index, row, vocabulary
index)`` (``parallel.rng.coupled_noise``), so a draft model and its target draw
token ``t`` with the same noise and speculative decoding can run under sampling.

``select_token`` is the whole per-token selection on the device (logits
processors, pick, EOS bookkeeping; ``Generation.device_loop``) on a
``SelectState``.  ``spec_verify`` is the verify step of a speculative
round (per-slot processors, picks, acceptance, EOS; ``Generation.spec_device_loop``)
on a ``SpecState``.
"""
import torch

from . import _lib
from ..parallel import rng


def fused_sample(logits, temperature=1.0, top_k=0, top_p=1.0, generator=None,
                 return_probs=False):
    """Sample one token per row of ``logits`` [B, V] (fp32 or bf16).

    Returns ``(ids int64 [B], lse fp32 [B])`` where ``lse`` is the logsumexp of
    the raw logits (the token log-prob is ``logits[ids] - lse``); with
    ``return_probs`` also the filtered, unnormalised probabilities [B, V]."""
    if logits.dim() != 2:
        raise ValueError("fused_sample expects [B, V] logits")
    B, V = logits.shape
    dev = logits.device
    if not logits.is_cuda:
        from ..models.language_model.gpt.generation import top_k_filter, top_p_filter
        lse = torch.logsumexp(logits.float(), -1)
        lg = logits.float() / temperature if temperature not in (None, 1.0) else logits.float()
        probs = torch.softmax(lg, -1)
        if top_k:
            probs = top_k_filter(probs, top_k)
        if top_p is not None and top_p < 1.0:
            probs = top_p_filter(probs, top_p)
        ids = torch.multinomial(probs, 1, generator=generator).squeeze(1)
        return (ids, lse, probs) if return_probs else (ids, lse)
    if logits.dtype == torch.float32:
        dc = 2
    elif logits.dtype == torch.bfloat16:
        dc = 0
    else:
        logits = logits.float()
        dc = 2
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    u = torch.rand(B, device=dev, generator=generator)
    ids = torch.empty(B, device=dev, dtype=torch.int64)
    lse = torch.empty(B, device=dev, dtype=torch.float32)
    probs = torch.empty(B, V, device=dev, dtype=torch.float32) if return_probs else None
    inv_t = 1.0 / float(temperature) if temperature not in (None, 0.0) else 1.0
    rc = _lib.kernels().sample(dc, logits.data_ptr(), logits.stride(0), B, V, inv_t,
                               int(top_k or 0), float(1.0 if top_p is None else top_p),
                               u.data_ptr(), ids.data_ptr(), lse.data_ptr(), _lib.ptr(probs),
                               _lib.stream())
    if rc != 0:
        raise RuntimeError("fused sampling launch failed ({})".format(rc))
    _lib.maybe_sync()
    return (ids, lse, probs) if return_probs else (ids, lse)


# ---------------------------------------------------------------------------
# the coupled sampler (coupled_sample_kernel in csrc/kernels/sampling.hip)
# ---------------------------------------------------------------------------
def seed_tensor(seed, device):
    """``seed`` as the int64 device tensor [1] the kernels read: a tensor is
    checked and kept, an int is wrapped to 64 bits."""
    if torch.is_tensor(seed):
        if seed.dtype != torch.int64 or seed.numel() != 1:
            raise ValueError("the seed tensor must be int64 with one element")
        return seed.to(device).view(1)
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([s - (1 << 64) if s >= 1 << 63 else s], dtype=torch.int64, device=device)


def coupled_keys(logits, temperature, top_k, top_p, seed, steps, rows=None, dtype=torch.float32):
    """The race of the coupled sampler as a PyTorch formula: ``keys`` [R, V] =
    ``logits / T + g`` on the tokens that ``top_k_filter`` / ``top_p_filter``
    keep and ``-inf`` elsewhere, with ``g = rng.coupled_noise(seed, steps[r],
    rows[r], V)``.  The pick is the argmax (lowest index among equal keys)."""
    from ..models.language_model.gpt.generation import top_k_filter, top_p_filter
    x = logits.float()
    R, V = x.shape
    temperature = 1.0 if temperature in (None, 0.0) else float(temperature)
    lg = x / temperature if temperature != 1.0 else x
    top_k = int(top_k or 0)
    top_p = 1.0 if top_p is None else float(top_p)
    if rows is None:
        rows = torch.arange(R)
    g = rng.coupled_noise(seed, steps, rows, V, device=x.device, dtype=dtype)
    keys = lg.to(dtype) + g
    if top_k or top_p < 1.0:
        probs = torch.softmax(lg, -1)
        if top_k:
            probs = top_k_filter(probs, top_k)
        if top_p < 1.0:
            probs = top_p_filter(probs, top_p)
        keys = torch.where(probs > 0, keys, torch.full_like(keys, float("-inf")))
    return keys


def coupled_sample(logits, temperature, top_k, top_p, seed, steps, rows=None, return_keys=False):
    """The coupled pick of one token per row of ``logits`` [R, V] (fp32): row
    ``r`` chooses token index ``steps[r]`` of noise row ``rows[r]`` (``r``
    itself without ``rows``): ``argmax_i (logits[r, i] / T + g_i)`` over the
    kept set of ``fused_sample`` with the shared noise ``g`` of
    ``rng.coupled_noise``.  ``seed`` is an int64 device tensor [1] (an int is
    wrapped), ``steps`` / ``rows`` int32 [R]; all three are read on the device,
    so a captured call follows them under graph replay.

    Returns ``(ids int64 [R], lse fp32 [R])`` as ``fused_sample`` does; with
    ``return_keys`` also the formula's keys [R, V] (``coupled_keys``).  CPU
    tensors take the formula."""
    if logits.dim() != 2:
        raise ValueError("coupled_sample expects [R, V] logits")
    R, V = logits.shape
    dev = logits.device
    seed = seed_tensor(seed, dev)
    steps = torch.as_tensor(steps, device=dev).to(torch.int32).reshape(-1).contiguous()
    if rows is not None:
        rows = torch.as_tensor(rows, device=dev).to(torch.int32).reshape(-1).contiguous()
    if steps.numel() != R or (rows is not None and rows.numel() != R):
        raise ValueError("coupled_sample expects %d steps and rows" % R)
    keys = None
    if return_keys or not logits.is_cuda:
        keys = coupled_keys(logits, temperature, top_k, top_p, seed, steps, rows)
    if not logits.is_cuda:
        ids = torch.argmax(keys, -1)
        lse = torch.logsumexp(logits.float(), -1)
        return (ids, lse, keys) if return_keys else (ids, lse)
    if logits.dtype != torch.float32 or logits.stride(1) != 1:
        logits = logits.float().contiguous()
    ids = torch.empty(R, device=dev, dtype=torch.int64)
    lse = torch.empty(R, device=dev, dtype=torch.float32)
    inv_t = 1.0 / float(temperature) if temperature not in (None, 0.0) else 1.0
    rc = _lib.kernels().coupled_sample(
        logits.data_ptr(), logits.stride(0), R, V, inv_t, int(top_k or 0),
        float(1.0 if top_p is None else top_p), steps.data_ptr(), _lib.ptr(rows),
        seed.data_ptr(), ids.data_ptr(), lse.data_ptr(), _lib.stream())
    if rc != 0:
        raise RuntimeError("coupled sampling launch failed ({})".format(rc))
    _lib.maybe_sync()
    return (ids, lse, keys) if return_keys else (ids, lse)


# ---------------------------------------------------------------------------
# on-device token selection (K18, K19; select_kernel in csrc/kernels/sampling.hip)
# ---------------------------------------------------------------------------
def _pack_seen(tokens, vocab):
    """Bitmap int32 [B, ceil(V/32)] (read as uint32 words) of the tokens in each
    row of ``tokens`` [B, n]; the ``V % 32`` tail bits stay 0."""
    B = tokens.shape[0]
    words = (vocab + 31) // 32
    bits = torch.zeros(B, words * 32, dtype=torch.bool, device=tokens.device)
    bits.scatter_(1, tokens, True)
    return _pack_bits(bits)


def _pack_bits(bits):
    """The bitmap of the boolean set ``bits`` [B, words * 32]."""
    B = bits.shape[0]
    w = (bits.view(B, -1, 32).long() << torch.arange(32, device=bits.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_seen(seen, vocab):
    """The boolean set [B, V] that the bitmap ``seen`` holds."""
    sh = torch.arange(32, device=seen.device, dtype=torch.int32)
    bits = (seen[:, :, None] >> sh) & 1
    return bits.bool().view(seen.shape[0], -1)[:, :vocab]


class SelectState:
    """The device-resident state of one ``generate()`` call's token selection
    (``select_token``); every tensor lives on ``input_ids``' device.

    * ``seen`` int32 [B, ceil(V/32)]: bitmap (uint32 words) of each row's
      history: all prompt columns, padding included, plus every emitted
      token, pads included -- what ``RepetitionPenaltyLogitsProcessor`` sees;
    * ``step`` int32 [B]: selections made so far; ``unfinished`` int32 [B];
      ``finish_len`` int32 [B] (``n_steps`` until the row emits EOS);
    * ``scores`` fp32 [B]; ``out`` int64 [B, n_steps];
    * ``nxt`` / ``cur`` int64 [B]: the token to embed next and its position
      ``lens + step`` -- the decode step's static inputs;
    * ``u`` fp32 [n_steps, B]: the uniforms of a sampling run;
    * ``seed`` int64 [1]: ``greedy=False`` with a ``seed`` and no ``u`` selects
      the coupled pick (``coupled_sample`` with token index ``step`` and the
      row's index) instead of the inverse-CDF draw.

    The scalars mirror ``GPTForGeneration._processors``: ``min_len`` (with an
    ``eos``), ``penalty``, ``forced_bos`` at step 0, ``forced_eos`` at step
    ``max_len - 1`` (``max_len`` defaults to ``n_steps``)."""

    def __init__(self, input_ids, lens, vocab, n_steps, greedy=True, temperature=1.0, top_k=0,
                 top_p=1.0, eos=None, pad=0, min_len=0, penalty=1.0, forced_bos=None,
                 forced_eos=None, max_len=None, u=None, seed=None):
        dev = input_ids.device
        B = input_ids.shape[0]
        if not 0 <= pad < vocab:
            raise ValueError("pad token %d outside the vocabulary" % pad)
        for t in (eos, forced_bos, forced_eos):
            if t is not None and not 0 <= t < vocab:
                raise ValueError("token %d outside the vocabulary" % t)
        self.coupled = not greedy and u is None and seed is not None
        if not greedy and not self.coupled and (u is None or tuple(u.shape) != (n_steps, B)):
            raise ValueError("sampling needs uniforms u [n_steps, B]")
        self.seed = seed_tensor(seed, dev) if self.coupled else None
        self.vocab, self.n_steps, self.greedy = vocab, n_steps, bool(greedy)
        self.temperature = 1.0 if temperature in (None, 0.0) else float(temperature)
        self.top_k = int(top_k or 0)
        self.top_p = float(1.0 if top_p is None else top_p)
        self.eos, self.pad = eos, pad
        self.min_len = int(min_len or 0) if eos is not None else 0
        self.penalty = float(penalty or 1.0)
        # the kernel's divide: torch's GPU `x / python_float` multiplies by the fp32 reciprocal
        self.inv_penalty = float(torch.tensor(1.0) / torch.tensor(self.penalty))
        self.forced_bos, self.forced_eos = forced_bos, forced_eos
        self.max_len = n_steps if max_len is None else int(max_len)
        self.u = None if u is None else u.to(dev, torch.float32).contiguous()
        self.lens = lens.to(dev, torch.long).contiguous()
        self.seen = _pack_seen(input_ids, vocab)
        self.step = torch.zeros(B, dtype=torch.int32, device=dev)
        self.unfinished = torch.ones(B, dtype=torch.int32, device=dev)
        self.finish_len = torch.full((B,), n_steps, dtype=torch.int32, device=dev)
        self.scores = torch.zeros(B, dtype=torch.float32, device=dev)
        self.out = torch.full((B, n_steps), pad, dtype=torch.long, device=dev)
        self.nxt = torch.zeros(B, dtype=torch.long, device=dev)
        self.cur = self.lens.clone()


def processed_logits(logits, state, step=None, seen=None):
    """The logits after the processors, as the selection sees them (PyTorch
    formula; does not change ``state``).  ``step`` [rows] and ``seen`` bool
    [rows, V] replace the state's step and history (a window slot of
    ``spec_verify``: its own step, the history plus its drafts)."""
    st = state
    x = logits.float().clone()
    step = st.step.long() if step is None else step.long()
    if st.min_len and st.eos is not None:
        x[:, st.eos] = torch.where(step < st.min_len, torch.full_like(x[:, 0], -1e9),
                                   x[:, st.eos])
    if st.penalty != 1.0:
        if seen is None:
            seen = unpack_seen(st.seen, st.vocab)
        x = torch.where(seen, torch.where(x < 0, x * st.penalty, x / st.penalty), x)
    for tok, at in ((st.forced_bos, 0), (st.forced_eos, st.max_len - 1)):
        if tok is not None:
            forced = torch.full_like(x, -1e9)
            forced[:, tok] = 0
            x = torch.where((step == at)[:, None], forced, x)
    return x


def select_token(logits, state):
    """One step of token selection on the device: the logits processors, the
    pick (greedy, top-k / top-p sampling with ``state.u[step]``, or the coupled
    pick of token index ``step`` under ``state.seed``) and the
    loop's bookkeeping, all from and into ``state`` (``SelectState``); nothing
    is read back to the host, so the call can be captured into a HIP graph
    behind the decode step.  ``logits`` [B, V] fp32 is not written.

    Per row, with ``unf = unfinished``: ``tok = pick if unf else pad``;
    ``scores += x'[pick] - logsumexp(x')`` if ``unf``; ``out[:, step] = tok``;
    ``seen`` gains ``tok``; an unfinished row that emits EOS clears
    ``unfinished`` and sets ``finish_len = step + 1``; ``nxt = tok``,
    ``cur = lens + step``, ``step += 1``.  A call at ``step >= n_steps`` does
    nothing.  Returns ``state.nxt``.

    GPU tensors run ``select_kernel`` (a missing extension raises); CPU
    tensors take the PyTorch formula with the same semantics."""
    st = state
    if logits.dim() != 2 or logits.shape[1] != st.vocab:
        raise ValueError("select_token expects [B, %d] logits" % st.vocab)
    B, V = logits.shape
    if logits.is_cuda:
        if logits.dtype != torch.float32 or logits.stride(1) != 1:
            logits = logits.float().contiguous()
        none = lambda t: -1 if t is None else int(t)  # noqa: E731
        rc = _lib.kernels().select(
            logits.data_ptr(), logits.stride(0), B, V,
            0 if st.greedy else 2 if st.coupled else 1,
            1.0 / st.temperature, st.top_k, st.top_p, _lib.ptr(st.u), st.n_steps, none(st.eos),
            st.pad, st.min_len, st.penalty, st.inv_penalty, none(st.forced_bos),
            none(st.forced_eos), st.max_len - 1, st.seen.data_ptr(), st.seen.shape[1],
            st.step.data_ptr(),
            st.unfinished.data_ptr(), st.finish_len.data_ptr(), st.scores.data_ptr(),
            st.out.data_ptr(), st.nxt.data_ptr(), st.cur.data_ptr(), st.lens.data_ptr(),
            _lib.stream(), _lib.ptr(st.seed))
        if rc != 0:
            raise RuntimeError("token selection launch failed ({})".format(rc))
        _lib.maybe_sync()
        return st.nxt
    step = st.step.long()
    live = step < st.n_steps
    if not bool(live.any()):
        return st.nxt
    x = processed_logits(logits, st)
    lse = torch.logsumexp(x, -1)
    if st.greedy:
        pick = torch.argmax(x, -1)
    elif st.coupled:
        pick = torch.argmax(coupled_keys(x, st.temperature, st.top_k, st.top_p, st.seed, step), -1)
    else:
        from ..models.language_model.gpt.generation import top_k_filter, top_p_filter
        probs = torch.softmax(x / st.temperature if st.temperature != 1.0 else x, -1)
        if st.top_k:
            probs = top_k_filter(probs, st.top_k)
        if st.top_p < 1.0:
            probs = top_p_filter(probs, st.top_p)
        # inverse CDF in index order: the first kept token whose running mass passes u * total
        c = torch.cumsum(probs, -1)
        u = st.u[step.clamp(max=st.n_steps - 1), torch.arange(B)]
        pick = (c <= (u * c[:, -1])[:, None]).sum(-1)
        last = (V - 1) - (probs > 0).flip(-1).long().argmax(-1)
        pick = torch.minimum(pick, last)
    unf = (st.unfinished != 0) & live
    tok = torch.where(unf, pick, torch.full_like(pick, st.pad))
    st.scores += torch.where(unf, x.gather(1, pick[:, None]).squeeze(1) - lse,
                             torch.zeros_like(lse))
    rows = torch.arange(B)[live]
    st.out[rows, step[live]] = tok[live]
    word = st.seen[rows, tok[live] >> 5].long() | \
        (torch.ones_like(rows) << (tok[live] & 31))
    st.seen[rows, tok[live] >> 5] = torch.where(word >= 2 ** 31, word - 2 ** 32,
                                                word).to(torch.int32)
    if st.eos is not None:
        fin = unf & (tok == st.eos)
        st.finish_len.copy_(torch.where(fin, (step + 1).int(), st.finish_len))
        st.unfinished.copy_(torch.where(fin, torch.zeros_like(st.unfinished), st.unfinished))
    st.nxt.copy_(torch.where(live, tok, st.nxt))
    st.cur.copy_(torch.where(live, st.lens + step, st.cur))
    st.step += live.int()
    return st.nxt


# ---------------------------------------------------------------------------
# on-device verify of speculative decoding (spec_pick_kernel and
# spec_accept_kernel in csrc/kernels/sampling.hip)
# ---------------------------------------------------------------------------
class SpecState(SelectState):
    """``SelectState`` of a speculative run (``spec_verify``): greedy, or
    with ``greedy=False`` and a ``seed`` the coupled pick (no inverse-CDF
    draw: its uniforms cannot be shared with a drafter).  ``step`` is the number of tokens emitted, ``nxt`` the last emitted
    token and ``cur`` its position (it is not in the KV cache yet).  On top of
    the base state, with ``W = window = spec_tokens + 1``:

    * ``tok`` / ``pos`` int64 [B*W]: the window step's static inputs; row
      ``b*W`` holds ``nxt[b]``, rows ``b*W + 1 ..`` the round's drafts, which
      the drafter writes; ``pos[b*W + j] = cur[b] + j``;
    * ``wlens`` int32 [B]: the keys before the window (``cur``);
    * ``picks`` int32 [B, W] / ``logp`` fp32 [B, W]: the target's pick
      of every slot and its log-probability (scratch between the two kernels);
    * ``rounds`` / ``accepted`` int32 [B]: rounds in which the row still
      emitted, and the drafts the target agreed with in them;
    * ``any_active`` int32 [1]: whether any row still emits.

    ``select_token`` on the prefill logits makes token 0; ``start_window``
    then fills the window inputs."""

    def __init__(self, input_ids, lens, vocab, n_steps, window, **kw):
        if not 1 <= window <= 8:
            raise ValueError("window must be in 1..8 (got %r)" % (window,))
        if input_ids.shape[0] > 64:
            raise ValueError("spec_verify covers at most 64 rows")
        greedy = kw.pop("greedy", True)
        if not greedy and (kw.get("u") is not None or kw.get("seed") is None):
            raise ValueError("a sampling SpecState needs a seed and no uniforms")
        super().__init__(input_ids, lens, vocab, n_steps, greedy=greedy, **kw)
        dev = input_ids.device
        B, W = input_ids.shape[0], int(window)
        self.window = W
        self.tok = torch.zeros(B * W, dtype=torch.long, device=dev)
        self.pos = torch.zeros(B * W, dtype=torch.long, device=dev)
        self.wlens = torch.zeros(B, dtype=torch.int32, device=dev)
        self.picks = torch.zeros(B, W, dtype=torch.int32, device=dev)
        self.logp = torch.zeros(B, W, dtype=torch.float32, device=dev)
        self.rounds = torch.zeros(B, dtype=torch.int32, device=dev)
        self.accepted = torch.zeros(B, dtype=torch.int32, device=dev)
        self.any_active = torch.zeros(1, dtype=torch.int32, device=dev)

    def active(self):
        """bool [B]: the rows that still emit."""
        return (self.unfinished != 0) & (self.step < self.n_steps)

    def start_window(self):
        """The first round's window inputs, from the state after token 0."""
        B, W = self.nxt.shape[0], self.window
        self.tok.view(B, W)[:, 0] = self.nxt
        self.pos.copy_((self.cur[:, None]
                        + torch.arange(W, device=self.cur.device)[None, :]).reshape(-1))
        self.wlens.copy_(self.cur)
        self.any_active.copy_(self.active().any().to(torch.int32).view(1))


def spec_verify(logits, state):
    """The verify step of one speculative round on the device: ``logits``
    [B*W, V] fp32 are the window step's (row ``b*W + j`` is slot ``j`` of
    sample ``b``; not written), the drafts ``d_1 .. d_g`` (``g = W - 1``) are
    in ``state.tok[b*W + 1 ..]``.  Everything comes from and goes into
    ``state`` (``SpecState``); nothing is returned or read back, so a whole
    round can be captured into one HIP graph.

    Per row, if ``unfinished`` and ``step < n_steps`` (any other row is left
    unchanged):

    * slot ``j`` chooses token ``step + j``: the processors act with that step
      (min length iff ``step + j < min_len``, forced EOS iff ``step + j ==
      max_len - 1``, never forced BOS) and the repetition penalty sees
      ``seen`` plus ``d_1 .. d_j`` (ids outside the vocabulary count as not
      seen; the bitmap itself is not touched); ``picks[j]`` is the argmax
      (lowest index among equal maxima) or, on a coupled state, the coupled
      pick of token index ``step + j`` in row ``b``;
      ``logp[j] = x'[pick] - logsumexp(x')``.
      Slots at or past ``n_steps`` are picked too and never emitted;
    * ``n`` = the leading ``i`` in ``1..g`` with ``d_i == picks[i-1]``;
      ``m = min(n + 1, n_steps - step)``; an EOS among ``picks[:m]`` cuts ``m``
      after its first occurrence, clears ``unfinished`` and sets
      ``finish_len = step + m``;
    * for ``j < m``: ``out[step + j] = picks[j]``, ``seen`` gains it,
      ``scores += logp[j]``;
    * ``nxt = picks[m-1]``, ``step += m``, ``cur += m``, ``rounds += 1``,
      ``accepted += n``; the next window's ``tok[b*W] = nxt``,
      ``pos[b*W + j] = cur + j``, ``wlens = cur``.

    ``any_active[0]`` = whether any row still emits after the round.

    GPU tensors run the two kernels (a missing extension raises); CPU tensors
    take the PyTorch formula with the same semantics."""
    st = state
    B, W, V = st.nxt.shape[0], st.window, st.vocab
    if logits.dim() != 2 or tuple(logits.shape) != (B * W, V):
        raise ValueError("spec_verify expects [%d, %d] logits" % (B * W, V))
    if logits.is_cuda:
        if logits.dtype != torch.float32 or logits.stride(1) != 1:
            logits = logits.float().contiguous()
        none = lambda t: -1 if t is None else int(t)  # noqa: E731
        rc = _lib.kernels().spec_verify(
            logits.data_ptr(), logits.stride(0), B, W, V, st.n_steps, none(st.eos), st.pad,
            st.min_len, st.penalty, st.inv_penalty, none(st.forced_eos), st.max_len - 1,
            st.seen.data_ptr(), st.seen.shape[1], st.step.data_ptr(), st.unfinished.data_ptr(),
            st.finish_len.data_ptr(), st.scores.data_ptr(), st.out.data_ptr(), st.nxt.data_ptr(),
            st.cur.data_ptr(), st.tok.data_ptr(), st.pos.data_ptr(), st.wlens.data_ptr(),
            st.picks.data_ptr(), st.logp.data_ptr(), st.rounds.data_ptr(),
            st.accepted.data_ptr(), st.any_active.data_ptr(), _lib.stream(),
            1 if st.coupled else 0, 1.0 / st.temperature, st.top_k, st.top_p, _lib.ptr(st.seed))
        if rc != 0:
            raise RuntimeError("speculative verify launch failed ({})".format(rc))
        _lib.maybe_sync()
        return
    g = W - 1
    step = st.step.long()
    active = st.active()
    lg = logits.float().view(B, W, V)
    d = st.tok.view(B, W)[:, 1:]
    ar = torch.arange(W)
    rows = torch.arange(B)
    # ---- the picks: slot j sees the history plus d_1 .. d_j
    seen = unpack_seen(st.seen, V)
    t = torch.zeros(B, W, dtype=torch.long)
    lp = torch.zeros(B, W)
    for j in range(W):
        if j:
            ok = (d[:, j - 1] >= 0) & (d[:, j - 1] < V)
            seen = seen.clone()
            seen[rows[ok], d[ok, j - 1]] = True
        x = processed_logits(lg[:, j], st, step + j, seen)
        if st.coupled:
            t[:, j] = torch.argmax(coupled_keys(x, st.temperature, st.top_k, st.top_p, st.seed,
                                                step + j), -1)
        else:
            t[:, j] = torch.argmax(x, -1)
        lp[:, j] = x.gather(1, t[:, j:j + 1]).squeeze(1) - torch.logsumexp(x, -1)
    st.picks.copy_(torch.where(active[:, None], t.int(), st.picks))
    st.logp.copy_(torch.where(active[:, None], lp, st.logp))
    # ---- accept
    n = (d == t[:, :g]).long().cumprod(1).sum(1)
    m = torch.minimum(n + 1, st.n_steps - step)
    m = torch.where(active, m, torch.zeros_like(m))
    emit = ar[None, :] < m[:, None]
    if st.eos is not None:
        hit = emit & (t == st.eos)
        done = hit.any(1)
        first = torch.where(hit, ar[None, :], W).min(1).values
        m = torch.where(done, first + 1, m)
        emit = ar[None, :] < m[:, None]
        st.finish_len.copy_(torch.where(done, (step + m).int(), st.finish_len))
        st.unfinished.copy_(torch.where(done, torch.zeros_like(st.unfinished), st.unfinished))
    # W slack columns: a window may reach past the last emitted token
    out = torch.cat([st.out, torch.zeros(B, W, dtype=torch.long)], 1)
    idx = step[:, None] + ar[None, :]
    out.scatter_(1, idx, torch.where(emit, t, out.gather(1, idx)))
    st.out.copy_(out[:, :st.n_steps])
    bits = torch.zeros(B, st.seen.shape[1] * 32, dtype=torch.bool)
    bits[:, :V] = unpack_seen(st.seen, V)
    er, ec = emit.nonzero(as_tuple=True)
    bits[er, t[er, ec]] = True
    st.seen.copy_(_pack_bits(bits))
    for j in range(W):  # in slot order, as the kernel adds
        st.scores += torch.where(emit[:, j], lp[:, j], torch.zeros_like(lp[:, j]))
    last = t.gather(1, (m - 1).clamp(min=0)[:, None]).squeeze(1)
    st.nxt.copy_(torch.where(active, last, st.nxt))
    st.step += m.int()
    st.cur += m
    st.rounds += active.int()
    st.accepted += torch.where(active, n, torch.zeros_like(n)).int()
    st.tok.view(B, W)[:, 0] = torch.where(active, st.nxt, st.tok.view(B, W)[:, 0])
    st.pos.copy_(torch.where(active[:, None], st.cur[:, None] + ar[None, :],
                             st.pos.view(B, W)).reshape(-1))
    st.wlens.copy_(torch.where(active, st.cur.int(), st.wlens))
    st.any_active.copy_(st.active().any().to(torch.int32).view(1))
