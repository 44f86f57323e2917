"""Autoregressive generation for GPT with a preallocated KV cache.

Parity: reference ``GPTForGeneration`` (``single_model.py:656-1122``, C27)
and its logits processors (``gpt/dygraph/processor.py:22-200``): min-length,
repetition penalty, Hamming diversity, forced BOS/EOS; sampling with
temperature / top-k / top-p + multinomial, and greedy search; per-token score
bookkeeping; stop when every sequence has produced EOS.  The hybrid (TP)
variant works here (reference defect §2.12 #1): logits are gathered over the
mp group before sampling.

MI355X design (K18/K19):
* prompts are RIGHT-padded and carried with per-sample lengths; the prefill
  runs the fused flash-attention kernel with ``kv_lens``, so no additive
  mask tensor is built;
* the KV cache is allocated once, ``[layers][B, max_len, heads, d]``, and each
  step writes one row per sample in place (no concat / re-allocation as in the
  reference ``_forward_`` path);
* per-token attention uses the split-free decode kernel
  (``ops.decode_attention``) that streams the cache once;
* a prompt longer than ``prefill_chunk`` tokens is prefilled in chunks over
  the cache, and a ``GenerationSession`` keeps the cache between
  ``generate()`` calls so a follow-up turn prefills only its new tokens
  (``ops.prefill_attention``: causal attention of a query block that starts
  at a per-sample cache offset);
* beam search (which the reference accepts and then raises on) keeps the
  prompt's K/V once per sample and the beams as an ancestor table
  (``BeamKVCache``, ``ops.beam_decode_attention``): a reorder moves no K/V;
* speculative greedy decoding (``spec_draft`` / ``set_drafter``) drafts on
  quantised copies of the model's own weights and verifies ``spec_tokens + 1``
  positions per sample in one window step of the target weights (a cache-row
  map in the QKV GEMV epilogue, ``ops.window_decode_attention``): the target's
  ids and scores, whatever the drafter proposes.  With ``spec_device_loop``
  the per-slot processors, picks, acceptance and EOS bookkeeping run in two
  kernels behind the window step (``ops.spec_verify``) and a whole round is
  one HIP graph replay;
* ``sampler: coupled`` draws every sampled token as a Gumbel race with noise
  that depends only on (seed, token index, row, vocabulary index)
  (``ops.coupled_sample``), so draft and target draw with the same noise and
  the speculative loops above run under ``decode_strategy: sampling`` as they
  do under greedy search: a draft is accepted iff it equals the target's pick.
"""
import os
import warnings

import torch
import torch.nn.functional as F

from .... import ops
from ....parallel import mappings as M
from ....parallel import topology as topo


# ----------------------------------------------------------------------------
# logits processors
# ----------------------------------------------------------------------------
class LogitsProcessor:
    def __call__(self, input_ids, logits):
        raise NotImplementedError


class LogitsProcessorList(list):
    def __call__(self, input_ids, logits, **kw):
        for p in self:
            logits = p(input_ids, logits)
        return logits


class MinLengthLogitsProcessor(LogitsProcessor):
    def __init__(self, min_length, eos_token_id):
        self.min_length, self.eos = min_length, eos_token_id
        self.cur_len = None

    def __call__(self, input_ids, logits):
        if self.cur_len is not None and self.cur_len < self.min_length:
            logits[:, self.eos] = -1e9
        return logits


class RepetitionPenaltyLogitsProcessor(LogitsProcessor):
    def __init__(self, penalty):
        assert penalty > 0
        self.penalty = penalty

    def __call__(self, input_ids, logits):
        score = torch.gather(logits, 1, input_ids)
        score = torch.where(score < 0, score * self.penalty, score / self.penalty)
        logits.scatter_(1, input_ids, score)
        return logits


class HammingDiversityLogitsProcessor(LogitsProcessor):
    """Penalise tokens chosen by earlier groups at this step (beam groups)."""

    def __init__(self, diversity_rate, num_beams, num_beam_groups):
        self.rate = diversity_rate
        self.group_size = num_beams // num_beam_groups
        self.num_beam_groups = num_beam_groups
        self.previous_tokens = None

    def __call__(self, input_ids, logits):
        if self.previous_tokens is None or self.rate == 0:
            return logits
        freq = torch.zeros_like(logits)
        freq.scatter_add_(1, self.previous_tokens, torch.ones_like(self.previous_tokens, dtype=logits.dtype))
        return logits - self.rate * freq


class ForcedBOSTokenLogitsProcessor(LogitsProcessor):
    def __init__(self, bos_token_id):
        self.bos = bos_token_id
        self.step = 0

    def __call__(self, input_ids, logits):
        if self.step == 0:
            logits[:] = -1e9
            logits[:, self.bos] = 0
        self.step += 1
        return logits


class ForcedEOSTokenLogitsProcessor(LogitsProcessor):
    def __init__(self, max_length, eos_token_id):
        self.max_length, self.eos = max_length, eos_token_id
        self.cur_len = None

    def __call__(self, input_ids, logits):
        if self.cur_len is not None and self.cur_len == self.max_length - 1:
            logits[:] = -1e9
            logits[:, self.eos] = 0
        return logits


def top_k_filter(probs, k, min_keep=1):
    k = min(max(k, min_keep), probs.shape[-1])
    kth = torch.topk(probs, k, dim=-1).values[:, -1:]
    return torch.where(probs >= kth, probs, torch.zeros_like(probs))


def top_p_filter(probs, p, min_keep=1):
    sp, si = torch.sort(probs, descending=True, dim=-1)
    cum = torch.cumsum(sp, dim=-1)
    remove = cum > p
    if min_keep > 1:
        remove[:, :min_keep - 1] = False
    remove[:, 1:] = remove[:, :-1].clone()
    remove[:, 0] = False
    mask = torch.zeros_like(remove).scatter(1, si, remove)
    return torch.where(mask, torch.zeros_like(probs), probs)


def _topk_ties_low(x, k):
    """Top ``k`` of each row of ``x`` [B, N], highest first, equal values in
    order of increasing index (``torch.topk`` leaves the order of ties open).
    Returns (values, indices)."""
    N = x.shape[1]
    v1, i1 = torch.topk(x, k, dim=1)
    kth = v1[:, -1:]
    # entries above the k-th value are certain; the rest are the lowest indices equal to it
    rev = N - torch.arange(N, device=x.device)
    v2, _ = torch.topk(torch.where(x == kth, rev, torch.zeros_like(rev)), k, dim=1)
    ninf = torch.full_like(v1, float("-inf"))
    vals = torch.cat([torch.where(v1 > kth, v1, ninf),
                      torch.where(v2 > 0, kth.expand_as(v1), ninf)], 1)
    idxs = torch.cat([i1, N - v2], 1)
    idxs, o = torch.sort(idxs, 1)
    vals, o = torch.sort(vals.gather(1, o), dim=1, descending=True, stable=True)
    return vals[:, :k], idxs.gather(1, o)[:, :k]


# ----------------------------------------------------------------------------
# cached decoding
# ----------------------------------------------------------------------------
class KVCache:
    def __init__(self, num_layers, batch, max_len, heads, head_dim, dtype, device):
        self.k = [torch.zeros(batch, max_len, heads, head_dim, dtype=dtype, device=device)
                  for _ in range(num_layers)]
        self.v = [torch.zeros_like(t) for t in self.k]
        self.max_len = max_len


class BeamKVCache:
    """KV cache for beam search: the prompt once per sample, the generated
    tokens as a tree.

    * ``k`` / ``v``: per-layer prefix ``[B, S, H, D]`` (``_layer_prefill`` fills
      it from the B prompts; it is never expanded to ``B*nb`` rows), with
      ``plens`` int32 ``[B]``;
    * ``kg`` / ``vg``: per-layer generated ``[B*nb, G, H, D]``; decode step
      ``t`` appends into slot ``t`` of every row;
    * ``anc`` int32 ``[B*nb, G]``: ``anc[b*nb+j, s]`` is the sample-local row
      whose slot ``s`` holds beam ``j``'s ancestor from step ``s``.  A beam
      reorder only gathers this table (``reorder``); no K/V byte moves.
    """

    def __init__(self, num_layers, batch, num_beams, prefix_len, gen_len, heads, head_dim, dtype,
                 device):
        self.k = [torch.zeros(batch, prefix_len, heads, head_dim, dtype=dtype, device=device)
                  for _ in range(num_layers)]
        self.v = [torch.zeros_like(t) for t in self.k]
        self.kg = [torch.zeros(batch * num_beams, gen_len, heads, head_dim, dtype=dtype,
                               device=device) for _ in range(num_layers)]
        self.vg = [torch.zeros_like(t) for t in self.kg]
        self.anc = torch.zeros(batch * num_beams, gen_len, dtype=torch.int32, device=device)
        self.plens = torch.zeros(batch, dtype=torch.int32, device=device)
        self.batch, self.num_beams, self.gen_len = batch, num_beams, gen_len
        self._self = torch.arange(num_beams, dtype=torch.int32, device=device)

    def reorder(self, parents, t):
        """Beam ``j`` of sample ``b`` continues beam ``parents[b, j]`` and will
        write its own K/V into slot ``t``: gather the parents' ancestor rows
        (through a temporary, so the update never reads its own writes), then
        point slot ``t`` at the row itself."""
        B, nb, G = self.batch, self.num_beams, self.gen_len
        new = self.anc.view(B, nb, G).gather(1, parents[:, :, None].expand(B, nb, G))
        new[:, :, t] = self._self
        self.anc.copy_(new.view(B * nb, G))


def _gen_kv(cache, li):
    """The caches a decode step appends to."""
    if isinstance(cache, BeamKVCache):
        return cache.kg[li], cache.vg[li]
    return cache.k[li], cache.v[li]


def _attend(cache, li, q, lens_after):
    """Single-token attention of ``q`` [rows, H, D] against layer ``li``.  For a
    ``BeamKVCache`` ``lens_after`` is ``glens`` [B], the valid generated slots."""
    if isinstance(cache, BeamKVCache):
        return ops.beam_decode_attention(q, cache.k[li], cache.v[li], cache.plens, cache.kg[li],
                                         cache.vg[li], lens_after, cache.anc)
    return ops.decode_attention(q, cache.k[li], cache.v[li], lens_after)


def _layer_prefill(layer, x, cache, li, lens):
    """Full-prompt pass of one decoder layer that also fills the KV cache."""
    attn = layer.attn
    h = layer.ln1(x)
    qkv = attn.qkv_proj(h)
    b, s = qkv.shape[0], qkv.shape[1]
    qkv5 = qkv.view(b, s, attn.heads, 3, attn.head_dim)
    cache.k[li][:, :s] = qkv5[:, :, :, 1]
    cache.v[li][:, :s] = qkv5[:, :, :, 2]
    o = ops.flash_attention(qkv5[:, :, :, 0], qkv5[:, :, :, 1], qkv5[:, :, :, 2], causal=True,
                            kv_lens=lens).reshape(b, s, -1)
    a, ab = attn.out_proj(o)
    x2, h2 = ops.add_layer_norm(a, ab, x, layer.ln2.weight, layer.ln2.bias, layer.ln2.eps)
    m, mb = layer.mlp(h2)
    return ops.bias_dropout_add(m, mb, x2)


def _layer_prefill_at(layer, x, cache, li, q_starts, kv_lens, rows, keep):
    """A block of new tokens per sample over a cache that holds their
    predecessors (a prefill chunk, a session turn): x [B, n, h]; token ``i`` of
    row ``b`` sits at position ``q_starts[b] + i`` and its K/V go to cache row
    ``rows[b, i]`` (the same number); ``kv_lens`` [B] keys are valid once the
    block is in.  ``keep``: None, or the (batch, token) index pair of the
    tokens whose cache row exists (padding tokens past the cache are dropped)."""
    attn = layer.attn
    h = layer.ln1(x)
    qkv = attn.qkv_proj(h)
    b, s = qkv.shape[0], qkv.shape[1]
    qkv5 = qkv.view(b, s, attn.heads, 3, attn.head_dim)
    kc, vc = cache.k[li], cache.v[li]
    if keep is None:
        ar = torch.arange(b, device=x.device)[:, None]
        kc[ar, rows] = qkv5[:, :, :, 1]
        vc[ar, rows] = qkv5[:, :, :, 2]
    else:
        bi, si = keep
        kc[bi, rows[bi, si]] = qkv5[bi, si, :, 1]
        vc[bi, rows[bi, si]] = qkv5[bi, si, :, 2]
    o = ops.prefill_attention(qkv5[:, :, :, 0], kc, vc, q_starts, kv_lens).reshape(b, s, -1)
    a, ab = attn.out_proj(o)
    x2, h2 = ops.add_layer_norm(a, ab, x, layer.ln2.weight, layer.ln2.bias, layer.ln2.eps)
    m, mb = layer.mlp(h2)
    return ops.bias_dropout_add(m, mb, x2)


class GenerationSession:
    """A conversation kept across ``generate(..., session=)`` calls
    (``GPTForGeneration.new_session``):

    * ``cache``: a ``KVCache`` of ``max_len`` rows;
    * ``lens`` [B]: tokens of each row's transcript whose K/V are in the cache;
    * ``pending`` [B]: the row's last emitted token, which is not in the cache
      yet (the next turn prefills it first), or -1;
    * ``tokens`` [B, max_len]: the transcript, ``lens + (pending >= 0)`` tokens
      per row (``history()`` pads it for the repetition penalty);
    * ``logits``: the fp32 [B, V] logits of the last prefill, the ones that
      choose the turn's first token.

    The position of a token is its index in the transcript."""

    def __init__(self, cache, batch_size, device):
        self.cache, self.batch_size, self.max_len = cache, batch_size, cache.max_len
        self.lens = torch.zeros(batch_size, dtype=torch.long, device=device)
        self.pending = torch.full((batch_size,), -1, dtype=torch.long, device=device)
        self.tokens = torch.zeros(batch_size, cache.max_len, dtype=torch.long, device=device)
        self.logits = None
        # host mirrors of lens / pending: the checks of a turn read no device memory
        self._lens, self._pending = [0] * batch_size, [-1] * batch_size

    def reset(self):
        """Forget the conversation; the cache rows are reused as they are."""
        self.lens.zero_()
        self.pending.fill_(-1)
        self.tokens.zero_()
        self.logits = None
        self._lens, self._pending = [0] * self.batch_size, [-1] * self.batch_size

    def history(self):
        """The transcript [B, L], L the longest row's length, padded with the
        row's own first token (a duplicate index that penalises nothing new)."""
        tl = self.lens + (self.pending >= 0).long()
        L = max(1, max(n + (p >= 0) for n, p in zip(self._lens, self._pending)))
        h = self.tokens[:, :L]
        return torch.where(torch.arange(L, device=h.device)[None, :] < tl[:, None], h, h[:, :1])

    def _put(self, tok, first, count):
        """tokens[b, first[b] + j] = tok[b, j] for j < count[b]."""
        valid = torch.arange(tok.shape[1], device=tok.device)[None, :] < count[:, None]
        bi, ji = valid.nonzero(as_tuple=True)
        self.tokens[bi, first[bi] + ji] = tok[bi, ji]


def _layer_decode(layer, x, cache, li, pos, lens_after, rows=None):
    """One-token pass: x [B, 1, h]; writes K/V at ``pos`` [B] and attends.  With
    a ``BeamKVCache`` ``pos`` is the generated slot per row and ``lens_after``
    the valid slots per sample.  Window form (``rows`` int32 [B*W], the cache
    row of every x row): x [B*W, 1, h], K/V go to ``cache[rows, pos]`` and
    ``lens_after`` [B] counts the keys before the window."""
    attn = layer.attn
    h = layer.ln1(x)
    qkv = attn.qkv_proj(h)
    b = qkv.shape[0]
    qkv5 = qkv.view(b, attn.heads, 3, attn.head_dim)
    ar = torch.arange(b, device=x.device) if rows is None else rows.long()
    kc, vc = _gen_kv(cache, li)
    kc[ar, pos] = qkv5[:, :, 1]
    vc[ar, pos] = qkv5[:, :, 2]
    if rows is None:
        o = _attend(cache, li, qkv5[:, :, 0].contiguous(), lens_after)
    else:
        o = ops.window_decode_attention(qkv5[:, :, 0].contiguous(), kc, vc, lens_after)
    a, ab = attn.out_proj(o.reshape(b, 1, -1))
    x2, h2 = ops.add_layer_norm(a, ab, x, layer.ln2.weight, layer.ln2.bias, layer.ln2.eps)
    m, mb = layer.mlp(h2)
    return ops.bias_dropout_add(m, mb, x2)


def _fusable(layer):
    from ....parallel import layers as L
    a, m = layer.attn, layer.mlp
    return (topo.mp_world_size() == 1 and type(a.qkv_proj) is L.ColumnParallelLinear
            and type(a.out_proj) is L.RowParallelLinear and type(m.fc1) is L.ColumnParallelLinear
            and type(m.fc2) is L.RowParallelLinear)


# LayerNorm as a GEMV prologue in the fused decode layer (FLEETX_DECODE_LN_FUSE=0: separate launch)
_LN_FUSE = os.environ.get("FLEETX_DECODE_LN_FUSE", "1") == "1"


# weight_quant value -> (quantiser in ops, its decode GEMV in ops.gemm, k-group
# size); a quantised copy is stored as (GEMV name, q, scale), so the format
# travels with it
_WEIGHT_QUANT = {"int8": ("quantize_weight_int8", "decode_linear_w8", 1),
                 "int4_g256": ("quantize_weight_int4", "decode_linear_w4", 256)}


def _qlin(G, x, q8, *args, **kw):
    """The decode GEMV of the quantised copy ``q8 = (GEMV name, q, scale)``."""
    return getattr(G, q8[0])(x, q8[1], q8[2], *args, **kw)


def _dlin(G, x, lin, epi, q8, **kw):
    """One decode GEMV of ``lin``: on its quantised copy ``q8`` where there is
    one and its kernel covers the call, else on the 16-bit weight."""
    if q8 is not None:
        y = _qlin(G, x, q8, lin.bias, epi, **kw)
        if y is not None:
            return y
    return G.decode_linear(x, lin.weight, lin.bias, epi, **kw)


def _layer_decode_fused(layer, x, cache, li, pos, lens_after, w8=None, rows=None):
    """One-token pass as four GEMV launches and the attention (K19, the
    fused_multi_transformer counterpart): [LN1 + QKV GEMV + bias, K/V appended
    to the cache in the epilogue] -> split-K decode attention -> [out-proj
    GEMV + bias + residual] -> [LN2 + FFN1 GEMV + bias + GeLU] -> [FFN2 GEMV +
    bias + residual].  The LayerNorms run as GEMV prologues (each block
    normalises the few rows into LDS); shapes the fused prologue does not
    cover fall back to a separate LayerNorm launch.  Returns None when a GEMV
    does not cover the shape (batch > 16).  ``w8`` (``weight_quant``) maps
    ``qkv_proj`` / ``out_proj`` / ``fc1`` / ``fc2`` to this layer's quantised copies.
    Window form (``rows`` int32 [B*W]): the QKV epilogue appends row ``m`` to
    ``cache[rows[m], pos[m]]`` and the attention is the window kernel with
    ``lens_after`` [B] keys before the window."""
    from ....ops import gemm as G
    attn, mlp = layer.attn, layer.mlp
    w8 = w8 or {}
    B, h = x.shape[0], x.shape[-1]
    x2d = x.reshape(B, h)
    kv = _gen_kv(cache, li) + ((pos,) if rows is None else (pos, rows))
    q = _dlin(G, x2d, attn.qkv_proj, G.GV_QKV, w8.get("qkv_proj"), qkv_cache=kv,
              ln=(layer.ln1.weight, layer.ln1.bias, layer.ln1.eps)) if _LN_FUSE else None
    if q is None:
        q = _dlin(G, layer.ln1(x2d), attn.qkv_proj, G.GV_QKV, w8.get("qkv_proj"), qkv_cache=kv)
    if q is None:
        return None
    if rows is None:
        o = _attend(cache, li, q.view(B, attn.heads, attn.head_dim), lens_after)
    else:
        o = ops.window_decode_attention(q.view(B, attn.heads, attn.head_dim), kv[0], kv[1],
                                        lens_after)
    x2 = _dlin(G, o.view(B, -1), attn.out_proj, G.GV_RES, w8.get("out_proj"), res=x2d)
    f = _dlin(G, x2, mlp.fc1, G.GV_GELU, w8.get("fc1"),
              ln=(layer.ln2.weight, layer.ln2.bias, layer.ln2.eps)) if _LN_FUSE else None
    if f is None:
        f = _dlin(G, layer.ln2(x2), mlp.fc1, G.GV_GELU, w8.get("fc1"))
    out = _dlin(G, f, mlp.fc2, G.GV_RES, w8.get("fc2"), res=x2)
    return out.view(B, 1, h)


class _GraphedDecodeStep:
    """The per-token decode step (embedding -> L decoder layers against the KV
    cache -> final LN -> logits) captured once into a HIP graph and replayed
    for every following token.

    At decode batch sizes every op is a tiny, launch-bound kernel (~10 per
    layer), so the eager loop is host-bound; a replay issues the whole step as
    one graph launch.  This is the MI355X counterpart of the reference's
    static inference program with ``fused_multi_transformer`` (K19 / N-12):
    the same fused HIP kernels, with the launch overhead removed by the graph
    instead of a tracing compiler.  The first call runs eagerly (it is also
    that token's real work) and captures; inputs live in static tensors.
    """

    def __init__(self, gen, cache, batch):
        self.gen, self.cache = gen, cache
        dev = cache.k[0].device
        self.nxt = torch.zeros(batch, dtype=torch.long, device=dev)
        self.cur = torch.zeros(batch, dtype=torch.long, device=dev)
        self.graph = None
        self.logits = None

    def __call__(self, nxt, cur):
        self.nxt.copy_(nxt)
        self.cur.copy_(cur)
        return self._capture_or_replay()

    def _capture_or_replay(self):
        """First call: run the step eagerly on a side stream (that token's real
        work) and capture it; afterwards replay.  Returns the step's output."""
        if self.graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):  # warm-up off the capture stream
                out = self._run()
            torch.cuda.current_stream().wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.logits = self._run()
            return out
        self.graph.replay()
        return self.logits

    def _run(self):
        return self.gen._decode_step(self.nxt, self.cur, self.cache)


class _GraphedBeamStep(_GraphedDecodeStep):
    """The beam decode step under the same capture-once / replay scheme.  Beyond
    tokens and positions, the slot, ``glens`` and the cache's ``anc`` table are
    static device tensors that the loop updates in place between replays."""

    def __init__(self, gen, cache, slot, glens):
        super().__init__(gen, cache, cache.batch * cache.num_beams)
        self.slot, self.glens = slot, glens

    def _run(self):
        return self.gen._beam_decode_step(self.nxt, self.cur, self.cache, self.slot, self.glens)


class _GraphedSelectStep(_GraphedDecodeStep):
    """Decode step and token selection (``ops.select_token``) as one graph:
    the selection writes the step's inputs ``nxt`` / ``cur`` itself (they are
    the state's tensors), so a token is one replay with no host copy and no
    host read."""

    def __init__(self, gen, cache, state):
        super().__init__(gen, cache, state.nxt.shape[0])
        self.state = state
        self.nxt, self.cur = state.nxt, state.cur

    def __call__(self):
        self._capture_or_replay()

    def _run(self):
        logits = self.gen._decode_step(self.nxt, self.cur, self.cache)
        ops.select_token(logits, self.state)
        return logits


class _GraphedWindowStep(_GraphedDecodeStep):
    """The window decode step (``_window_step``) under the same capture-once /
    replay scheme: tokens, cache positions and ``lens`` are static tensors; the
    row map is constant (row ``b*W + j`` belongs to sample ``b``)."""

    def __init__(self, gen, cache, batch, window):
        super().__init__(gen, cache, batch * window)
        dev = self.nxt.device
        self.rows = torch.arange(batch, dtype=torch.int32, device=dev).repeat_interleave(window)
        self.lens = torch.zeros(batch, dtype=torch.int32, device=dev)

    def __call__(self, tok, pos, lens):
        self.lens.copy_(lens)
        return super().__call__(tok, pos)

    def _run(self):
        return self.gen._window_step(self.nxt, self.cur, self.rows, self.lens, self.cache)


class _GraphedDraftStep(_GraphedDecodeStep):
    """One draft token as one graph: a plain decode step on the draft copies
    (LM head included), the argmax, and the advance of the step's own inputs
    ``nxt`` / ``cur``, so ``k`` replays draft ``k`` tokens with no host work
    between them.  After ``couple(seed)`` the pick is the coupled one
    (``ops.coupled_sample`` on the raw draft logits) with the token index in
    the static tensor ``steps``, which advances with ``cur``."""

    steps = seed = None

    def couple(self, seed):
        self.seed = seed.clone()
        self.steps = torch.zeros(self.nxt.shape[0], dtype=torch.int32, device=self.nxt.device)

    def _run(self):
        gen, cur = self.gen, self.cur
        ids = cur.clamp(max=gen.gpt.cfg.max_position_embeddings - 1)
        logits = gen._step(self.nxt, ids, self.cache, cur, (cur + 1).to(torch.int32),
                           copies=gen._wd)
        if self.steps is None:
            self.nxt.copy_(torch.argmax(logits, -1))
        else:
            self.nxt.copy_(ops.coupled_sample(logits, gen.temperature, gen.top_k, gen.top_p,
                                              self.seed, self.steps)[0])
            self.steps.add_(1)
        cur.add_(1)
        return logits


class _GraphedSpecRound(_GraphedDecodeStep):
    """One round of speculative decoding with the verify on the device
    (``spec_device_loop``) as one graph: with the built-in drafter
    (``draft``) the copy of ``state.nxt`` / ``state.cur`` into the draft
    step's inputs and ``spec_tokens`` draft steps, each writing its argmax
    into the window's tokens; then the window step on ``state.tok`` /
    ``state.pos`` / ``state.wlens`` and ``ops.spec_verify``, which writes the
    next round's inputs itself.  A round is one replay with no host copy and
    no host read.  Without ``draft`` (a ``set_drafter`` drafter fills
    ``state.tok`` from the host) the graph is {window step, verify}."""

    def __init__(self, gen, cache, state, draft):
        B, W = state.nxt.shape[0], state.window
        super().__init__(gen, cache, B * W)
        self.state = state
        self.nxt, self.cur = state.tok, state.pos
        self.rows = torch.arange(B, dtype=torch.int32,
                                 device=state.tok.device).repeat_interleave(W)
        self.draft = _GraphedDraftStep(gen, cache, B) if draft else None
        if draft and state.coupled:
            self.draft.couple(state.seed)

    def __call__(self):
        if self.gen.use_hip_graph and self.nxt.is_cuda:
            self._capture_or_replay()
        else:
            self._run()

    def _run(self):
        st, d = self.state, self.draft
        if d is not None:
            d.nxt.copy_(st.nxt)
            d.cur.copy_(st.cur)
            if d.steps is not None:  # draft i guesses token step + i - 1
                d.steps.copy_(st.step)
            tok = st.tok.view(-1, st.window)
            for i in range(st.window - 1):
                d._run()
                tok[:, i + 1].copy_(d.nxt)
        logits = self.gen._window_step(st.tok, st.pos, self.rows, st.wlens, self.cache)
        ops.spec_verify(logits, st)
        return logits


class _CoupledPick:
    """The ``pick`` of ``propose_coupled``: ``pick(logits [B, V], i)`` is the
    coupled pick for draft ``i`` in ``1..k``, a guess at token ``step + i - 1``.
    ``seed`` (int64 [1]) and ``step`` (the tokens emitted so far, [B]) are the
    run's device tensors."""

    def __init__(self, gen, seed, step):
        self.gen, self.seed, self.step = gen, seed, step

    def __call__(self, logits, i):
        g = self.gen
        return ops.coupled_sample(logits, g.temperature, g.top_k, g.top_p, self.seed,
                                  self.step.to(logits.device) + (i - 1))[0]


def _propose(drafter, last, cur, cache, k, pick):
    """The drafter's ``k`` tokens: ``propose_coupled`` under the coupled sampler
    if it defines one, else ``propose``."""
    if pick is not None and hasattr(drafter, "propose_coupled"):
        return drafter.propose_coupled(last, cur, cache, k, pick)
    return drafter.propose(last, cur, cache, k)


class _QuantDrafter:
    """The built-in drafter of speculative decoding: ``k`` greedy decode steps
    on the ``spec_draft`` copies of the model's own weights.  It writes its
    K/V into the shared cache at ``cur .. cur+k-1``; the verify step
    overwrites those rows with the target's."""

    def __init__(self, gen):
        self.gen = gen
        self.step = None

    def propose(self, last, cur, cache, k):
        return self.propose_coupled(last, cur, cache, k, None)

    def propose_coupled(self, last, cur, cache, k, pick):
        if self.step is None or self.step.cache is not cache:
            self.step = _GraphedDraftStep(self.gen, cache, last.shape[0])
            if pick is not None:
                self.step.couple(pick.seed)
        st = self.step
        st.nxt.copy_(last)
        st.cur.copy_(cur)
        if pick is not None:
            st.seed.copy_(pick.seed)
            st.steps.copy_(pick.step)
        out = torch.empty(last.shape[0], k, dtype=torch.long, device=last.device)
        for i in range(k):
            if self.gen.use_hip_graph:
                st._capture_or_replay()
            else:
                st._run()
            out[:, i] = st.nxt
        return out

    def release(self):
        self.step = None


class GPTForGeneration(torch.nn.Module):
    def __init__(self, pretrain_model, configs):
        super().__init__()
        self.model = pretrain_model  # GPTForPretraining
        self.gpt = pretrain_model.gpt
        c = configs or {}
        self.max_length = c.get("max_dec_len", 20)
        self.min_length = c.get("min_dec_len", 0)
        self.decode_strategy = c.get("decode_strategy", "sampling")
        # the sampling draw: inverse CDF with a uniform per row, or the coupled pick (a
        # Gumbel race with noise shared by index), under which speculation may sample
        self.sampler = c.get("sampler", "inverse_cdf")
        if self.sampler not in ("inverse_cdf", "coupled"):
            raise ValueError("sampler must be 'inverse_cdf' or 'coupled' (got %r)"
                             % (self.sampler,))
        self.temperature = c.get("temperature", 1.0)
        self.top_k = c.get("top_k", 0)
        self.top_p = c.get("top_p", 1.0)
        self.repetition_penalty = c.get("repetition_penalty", 1.0)
        self.num_beams = c.get("num_beams", 1)
        self.num_beam_groups = c.get("num_beam_groups", 1)
        self.diversity_rate = c.get("diversity_rate", 0.0)
        self.bos_token_id = c.get("bos_token_id")
        self.eos_token_id = c.get("eos_token_id")
        self.pad_token_id = c.get("pad_token_id")
        self.forced_bos_token_id = c.get("forced_bos_token_id")
        self.forced_eos_token_id = c.get("forced_eos_token_id")
        self.num_return_sequences = c.get("num_return_sequences", 1)
        self.use_hip_graph = bool(c.get("use_hip_graph", True))
        # decode layers as five fused kernels with weight-streaming GEMVs (K19)
        self.fused_decode = bool(c.get("fused_decode", True))
        self.length_penalty = c.get("length_penalty", 0.0)
        self.early_stopping = bool(c.get("early_stopping", False))
        # weight-only int8 / int4 copies of the decode GEMV weights (None: 16-bit weights)
        self.weight_quant = c.get("weight_quant")
        if self.weight_quant is not None and self.weight_quant not in _WEIGHT_QUANT:
            raise ValueError("weight_quant must be None, %s (got %r)"
                             % (" or ".join(repr(k) for k in _WEIGHT_QUANT), self.weight_quant))
        self._w8 = None        # {"layers": [{name: (GEMV name, q, scale)}], "head": (...)}
        self._w8_src = []      # (weight, _version, data_ptr) of every quantised weight
        self._w8_warned = False
        # token selection on the device, one graph replay per token (sampling / greedy)
        self.device_loop = bool(c.get("device_loop", False))
        self.eos_poll = max(1, int(c.get("eos_poll", 8)))
        self._device_loop_warned = False
        if self.decode_strategy not in ("sampling", "greedy_search", "beam_search"):
            raise ValueError("decode_strategy must be sampling, greedy_search or beam_search")
        # prompts longer than this are prefilled in chunks of this many tokens (0: one pass)
        self.prefill_chunk = c.get("prefill_chunk", 0)
        if isinstance(self.prefill_chunk, bool) or not isinstance(self.prefill_chunk, int) \
                or self.prefill_chunk < 0 or self.prefill_chunk % 64:
            raise ValueError("prefill_chunk must be 0 or a positive multiple of 64 (got %r)"
                             % (self.prefill_chunk,))
        # speculative greedy decoding: draft on quantised copies, verify spec_tokens + 1
        # positions in one window step of the target weights
        self.spec_draft = c.get("spec_draft")
        self.spec_tokens = int(c.get("spec_tokens", 4))
        self._wd = None        # the draft's copies, laid out like _w8
        self._drafter = None   # installed by set_drafter
        self._quant_drafter = None
        self._spec_warned = False
        self.last_spec_stats = None
        if self.spec_draft is not None:
            if self.spec_draft not in _WEIGHT_QUANT:
                raise ValueError("spec_draft must be None, %s (got %r)"
                                 % (" or ".join(repr(k) for k in _WEIGHT_QUANT), self.spec_draft))
            if self.spec_draft == self.weight_quant:
                raise ValueError("spec_draft must differ from weight_quant (%r): a draft in the "
                                 "target's format saves nothing" % (self.weight_quant,))
            self._spec_check()
        # the speculative loop with the verify on the device, one graph replay per round;
        # any_active is read every spec_poll rounds
        self.spec_device_loop = bool(c.get("spec_device_loop", False))
        self.spec_poll = max(1, int(c.get("spec_poll", 1)))
        if self.spec_device_loop:
            self._spec_check()
        if self.decode_strategy == "beam_search":
            if self.num_beam_groups > 1:
                raise ValueError("diverse beam search (num_beam_groups > 1) is not supported yet")
            if self.num_beams < 1:
                raise ValueError("num_beams must be at least 1")
            if self.num_return_sequences > self.num_beams:
                raise ValueError("num_return_sequences (%d) must not exceed num_beams (%d)"
                                 % (self.num_return_sequences, self.num_beams))

    def _spec_check(self):
        if not 1 <= self.spec_tokens <= 7:
            raise ValueError("spec_tokens must be in 1..7 (got %r)" % (self.spec_tokens,))
        if not (self.decode_strategy == "greedy_search" or self._coupled()) or self.device_loop \
                or self.num_return_sequences > 1:
            raise ValueError("speculative decoding supports greedy_search, or sampling with "
                             "sampler: coupled, without device_loop and with "
                             "num_return_sequences 1")

    def _coupled(self):
        return self.decode_strategy == "sampling" and self.sampler == "coupled"

    def _coupled_seed(self, seed, dev):
        """The seed tensor of a coupled run (None otherwise): ``generate(seed=)``,
        or one drawn from torch's default generator."""
        if not self._coupled():
            return None
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        return ops.sampling.seed_tensor(seed, dev)

    def set_drafter(self, drafter):
        """Install the drafter of speculative decoding (any device): an
        object with ``propose(last, cur, cache, k) -> LongTensor [B, k]``, the
        ``k`` tokens it expects after ``last`` [B], which sits at position
        ``cur`` [B] and is not in ``cache`` yet.  It may write cache rows
        ``cur .. cur+k-1``; the verify step overwrites them.  The output is
        the target's whatever it proposes.  Under ``sampler: coupled`` a
        drafter that defines ``propose_coupled(last, cur, cache, k, pick)`` is
        asked through it: ``pick(logits [B, V], i)`` is the coupled pick for
        draft ``i`` in ``1..k`` (the target's own noise for that token, so a
        draft model close to the target is accepted as often as the coupling
        allows).  ``None`` removes it."""
        if drafter is not None:
            self._spec_check()
        self._drafter = drafter

    def _processors(self, max_len):
        procs = LogitsProcessorList()
        if self.min_length and self.eos_token_id is not None:
            procs.append(MinLengthLogitsProcessor(self.min_length, self.eos_token_id))
        if self.repetition_penalty and self.repetition_penalty != 1.0:
            procs.append(RepetitionPenaltyLogitsProcessor(self.repetition_penalty))
        if self.num_beam_groups > 1 and self.diversity_rate > 0:
            procs.append(HammingDiversityLogitsProcessor(self.diversity_rate, self.num_beams,
                                                         self.num_beam_groups))
        if self.forced_bos_token_id is not None:
            procs.append(ForcedBOSTokenLogitsProcessor(self.forced_bos_token_id))
        if self.forced_eos_token_id is not None:
            procs.append(ForcedEOSTokenLogitsProcessor(max_len, self.forced_eos_token_id))
        return procs

    # ---- weight-only quantised decode (weight_quant: int8 / int4_g256)
    def _w8_sources(self):
        """The weights the decode step streams: four per fusable layer and the
        tied embedding table (as the LM head)."""
        per_layer = []
        for layer in self.gpt.layers:
            per_layer.append({"qkv_proj": layer.attn.qkv_proj.weight,
                              "out_proj": layer.attn.out_proj.weight,
                              "fc1": layer.mlp.fc1.weight, "fc2": layer.mlp.fc2.weight}
                             if _fusable(layer) else {})
        return per_layer, self.gpt.embeddings.word_embeddings.weight

    def requantize(self):
        """(Re)build the quantised copies from the current 16-bit weights: the
        target's (``weight_quant``) and the draft's (``spec_draft``).  The
        16-bit weights stay resident (prefill and the embedding lookup use
        them): the quantised path buys decode bandwidth, not memory.  Returns
        True when the quantised path is active; on CPU or under tensor parallel
        the keys are accepted and ignored with one warning (those paths do not
        stream weights through the decode GEMV).  A weight the format cannot
        hold (int4: K no multiple of the group size) keeps no copy and decodes
        on its 16-bit weight."""
        if self.weight_quant is None and self.spec_draft is None:
            return False
        head = self.gpt.embeddings.word_embeddings.weight
        if not head.is_cuda or topo.mp_world_size() != 1 or not self.fused_decode:
            if self.weight_quant is not None and not self._w8_warned:
                warnings.warn("weight_quant=%r is ignored: the quantised decode path needs a GPU, "
                              "fused_decode and no tensor parallelism" % (self.weight_quant,))
                self._w8_warned = True
            self._w8, self._wd, self._w8_src = None, None, []
            return False
        per_layer, head = self._w8_sources()
        self._w8_src = [(w, w._version, w.data_ptr())
                        for w in [w for d in per_layer for w in d.values()] + [head]]

        def copies(fmt):
            if fmt is None:
                return None
            quantiser, gemv, group = _WEIGHT_QUANT[fmt]

            def quant(w):
                if w.shape[1] % group:
                    return None
                return (gemv,) + getattr(ops, quantiser)(w)
            return {"layers": [{k: quant(w) for k, w in d.items()} for d in per_layer],
                    "head": quant(head)}
        with torch.no_grad():
            self._w8, self._wd = copies(self.weight_quant), copies(self.spec_draft)
        return True

    def _w8_refresh(self):
        """At the start of ``generate()``: quantise on first use and whenever a
        source weight was written in place or replaced since."""
        if (self.weight_quant is None or self._w8_warned) and self.spec_draft is None:
            return
        stale = self._w8 is None and self._wd is None
        if not stale:
            cur = [w for d in self._w8_sources()[0] for w in d.values()]
            cur.append(self.gpt.embeddings.word_embeddings.weight)
            stale = len(cur) != len(self._w8_src) or any(
                w is not s or w._version != v or w.data_ptr() != p
                for w, (s, v, p) in zip(cur, self._w8_src))
        if stale:
            self.requantize()

    def _decode_step(self, nxt, cur, cache):
        """Embed token ``nxt`` at position ``cur`` [B], run every layer against
        the KV cache (appending this token), return fp32 logits [B, V]."""
        return self._step(nxt, cur, cache, cur, (cur + 1).to(torch.int32))

    def _beam_decode_step(self, nxt, pos, cache, slot, glens):
        """Beam decode step on a ``BeamKVCache``: embed token ``nxt`` [B*nb] at
        position ``pos`` [B*nb], append K/V into ``slot`` [B*nb] (the step
        number, the same for every row) of the generated caches, attend over
        the shared prefix and, through ``cache.anc``, ``glens`` [B] generated
        slots; return fp32 logits [B*nb, V]."""
        return self._step(nxt, pos, cache, slot, glens)

    def _window_step(self, tok, pos, rows, lens, cache):
        """Window decode step: ``W`` consecutive tokens per sample in one pass.
        ``tok`` [B*W] sits at cache position ``pos`` [B*W] (= ``lens[b] + j``)
        of cache row ``rows`` int32 [B*W] (= ``b``); ``lens`` int32 [B] keys
        precede the window.  Appends the B*W K/V rows and returns fp32 logits
        [B*W, V]; row ``b*W + j`` sees the cache up to its own position.
        Position ids past ``max_position_embeddings`` are clamped (such slots
        are never emitted)."""
        ids = pos.clamp(max=self.gpt.cfg.max_position_embeddings - 1)
        return self._step(tok, ids, cache, pos, lens, rows=rows)

    def _step(self, nxt, pos, cache, wpos, after, rows=None, copies=None):
        """``rows``: window form (see ``_window_step``).  ``copies``: the
        quantised copies to stream (default: the target's, ``weight_quant``)."""
        q8 = self._w8 if copies is None else copies
        x = ops.embedding(nxt[:, None], self.gpt.embeddings.word_embeddings.weight,
                          pos[:, None], self.gpt.embeddings.position_embeddings, 0) \
            if topo.mp_world_size() == 1 else self.gpt.embeddings(nxt[:, None], pos[:, None])
        fused = self.fused_decode and x.is_cuda and x.shape[0] <= 16
        w8 = q8["layers"] if q8 is not None else None
        for li, layer in enumerate(self.gpt.layers):
            if fused and _fusable(layer):
                y = _layer_decode_fused(layer, x, cache, li, wpos, after, w8[li] if w8 else None,
                                        rows)
            else:
                y = None
            x = y if y is not None else _layer_decode(layer, x, cache, li, wpos, after, rows)
        x = self.gpt.final_ln(x)
        return self._logits(x[:, 0], q8["head"] if q8 is not None else None)

    def _logits(self, h, q8=None):
        """``q8``: the quantised copy of the tied table (decode steps; the prefill's
        last-token logits use the 16-bit table like the rest of the prefill)."""
        w = self.gpt.embeddings.word_embeddings.weight
        logits = None
        if self.fused_decode and topo.mp_world_size() == 1:
            from ....ops import gemm as G
            if q8 is not None:
                logits = _qlin(G, h.contiguous(), q8)
            if logits is None:
                logits = G.decode_linear(h.contiguous(), w)
        if logits is None:
            logits = F.linear(h, w)
        if topo.mp_world_size() > 1:
            logits = M.gather_from_mp(logits)
        return logits.float()

    # ---- prefill
    def _prompt_logits(self, input_ids, lens, cache, lens32):
        """Prefill of the right-padded prompts into an empty ``cache`` and the
        fp32 logits of each row's last token: in one pass, or, for prompts
        longer than ``prefill_chunk``, in chunks."""
        B, S = input_ids.shape
        dev = input_ids.device
        if self.prefill_chunk and S > self.prefill_chunk:
            return self._prefill_at(input_ids, lens, [0] * B, cache)
        pos = torch.arange(S, device=dev).unsqueeze(0).expand(B, S)
        x = self.gpt.embeddings(input_ids, pos)
        for li, layer in enumerate(self.gpt.layers):
            x = _layer_prefill(layer, x, cache, li, lens32)
        x = self.gpt.final_ln(x)
        last = x[torch.arange(B, device=dev), lens - 1]
        return self._logits(last)

    def _prefill_at(self, tok, count, start, cache):
        """Prefill ``count[b]`` tokens ``tok[b, :count[b]]`` (right-padded
        [B, S]) at positions ``start[b] ..`` of a cache that holds each row's
        first ``start[b]`` tokens (``start``: host list), at most
        ``prefill_chunk`` tokens at a time (0: all at once).  Chunk ``c`` of
        row ``b`` starts at ``start[b] + c N`` and sees ``start[b] +
        min(count[b], (c + 1) N)`` keys; its K/V go to the cache rows of its
        positions.  Padding tokens are written too where their row exists:
        above the row's valid length, so never visible before the real token
        overwrites them.  Returns the fp32 logits [B, V] of each row's last
        token, taken from the chunk it falls in."""
        B, S = tok.shape
        dev = tok.device
        N = self.prefill_chunk or S
        nrows = cache.k[0].shape[1]
        start_t = torch.tensor(start, dtype=torch.long, device=dev)
        ar = torch.arange(B, device=dev)
        last_pos = count - 1
        last = None
        for c in range(-(-S // N)):
            n = min(N, S - c * N)
            q_starts = start_t + c * N
            kv_lens = (start_t + count.clamp(max=c * N + n)).to(torch.int32)
            rows = q_starts[:, None] + torch.arange(n, device=dev)[None, :]
            keep = None
            if max(start) + c * N + n > nrows:
                keep = (rows < nrows).nonzero(as_tuple=True)
            pos = rows.clamp(max=self.gpt.cfg.max_position_embeddings - 1)
            x = self.gpt.embeddings(tok[:, c * N:c * N + n], pos)
            q32 = q_starts.to(torch.int32)
            for li, layer in enumerate(self.gpt.layers):
                x = _layer_prefill_at(layer, x, cache, li, q32, kv_lens, rows, keep)
            here = (last_pos >= c * N) & (last_pos < c * N + n)
            xl = x[ar, (last_pos - c * N).clamp(0, n - 1)]
            last = xl if last is None else torch.where(here[:, None], xl, last)
        return self._logits(self.gpt.final_ln(last))

    def new_session(self, batch_size, max_len=None):
        """A ``GenerationSession`` of ``batch_size`` rows whose cache holds
        ``min(max_len or max_position_embeddings, max_position_embeddings)``
        tokens per row; pass it to ``generate(..., session=)`` turn by turn."""
        mpe = self.gpt.cfg.max_position_embeddings
        p = next(self.parameters())
        attn0 = self.gpt.layers[0].attn
        cache = KVCache(len(self.gpt.layers), batch_size, min(max_len or mpe, mpe), attn0.heads,
                        attn0.head_dim, p.dtype, p.device)
        return GenerationSession(cache, batch_size, p.device)

    def _session_turn(self, s, input_ids, lens):
        """Checks of a session turn (each a ``ValueError`` before anything is
        launched) and its tokens: ``[pending] + new tokens`` per row,
        right-padded [B, S'], with their counts (device and host)."""
        if self.decode_strategy == "beam_search" or self.device_loop or self.spec_device_loop \
                or self.spec_draft is not None or self._drafter is not None:
            raise ValueError("a session supports sampling and greedy_search in the host loop "
                             "only (no beam_search, device_loop or speculative decoding)")
        if self.num_return_sequences != 1:
            raise ValueError("a session needs num_return_sequences 1")
        B, S = input_ids.shape
        if B != s.batch_size:
            raise ValueError("batch size %d does not match the session's %d" % (B, s.batch_size))
        new = [S] * B if lens is None else [int(n) for n in lens.tolist()]
        if any(n < 0 or n > S for n in new):
            raise ValueError("lens must lie in 0..%d" % S)
        count = [n + (p >= 0) for n, p in zip(new, s._pending)]
        if any(n == 0 for n in count):
            raise ValueError("a row has neither a pending token nor new tokens")
        if any(a + n > s.max_len for a, n in zip(s._lens, count)):
            raise ValueError("the turn's tokens do not fit the session's %d rows" % s.max_len)
        dev = input_ids.device
        Sp = max(count)
        src = torch.cat([s.pending.clamp(min=0)[:, None], input_ids], 1)     # [B, S + 1]
        idx = torch.arange(Sp, device=dev)[None, :] + (s.pending < 0).long()[:, None]
        tok = src.gather(1, idx.clamp(max=S))
        return tok, torch.tensor(count, dtype=torch.long, device=dev), count

    @torch.no_grad()
    def generate(self, input_ids, lens=None, max_length=None, seed=None, session=None):
        """input_ids: [B, S] right-padded; lens: [B] prompt lengths.
        Returns (generated ids [B, T], scores [B]); with ``decode_strategy:
        beam_search`` see ``_beam_search``.

        With ``session`` (``new_session``) the call is one turn of a
        conversation: ``input_ids`` / ``lens`` are the turn's new tokens, only
        ``[pending] + new tokens`` of each row are prefilled, at offset
        ``session.lens`` over the session's cache (``ops.prefill_attention``),
        and the decode runs at the transcript's positions.  Afterwards a row
        that emitted ``n`` tokens (up to and including its EOS, pads excluded)
        has ``lens`` grown by the prefilled tokens plus ``n - 1`` and the
        ``n``-th token pending (``n = 0``: nothing pending).  Sampling and
        greedy search in the host loop only.

        With ``device_loop`` (sampling / greedy only) the processors, the pick
        and the EOS bookkeeping run in one kernel behind the decode step
        (``ops.select_token``) and the host reads ``unfinished`` only every
        ``eos_poll`` tokens; ids and scores are those of the default loop.
        Seeded sampling is reproducible under ``device_loop`` but draws its
        uniforms in a different order (one ``[N, B]`` table up front; on the
        CPU an inverse-CDF draw instead of ``torch.multinomial``), so a seed
        does not give the default loop's tokens.

        With ``sampler: coupled`` token ``t`` of row ``b`` (the row of the
        expanded batch) is the coupled pick of ``(seed, t, b)`` in every loop
        (host loop, ``device_loop``, sessions, the speculative loops), so a
        seed gives one text per path of logits; without ``seed`` one is drawn
        from torch's default generator."""
        self.eval()
        if session is not None:
            return self._generate_turn(session, input_ids, lens, max_length, seed)
        self._w8_refresh()  # before the prefill and any graph capture
        if self.decode_strategy == "beam_search":
            return self._beam_search(input_ids, lens, max_length)
        dev = input_ids.device
        if self.num_return_sequences > 1:
            input_ids = input_ids.repeat_interleave(self.num_return_sequences, 0)
            if lens is not None:
                lens = lens.repeat_interleave(self.num_return_sequences, 0)
        B, S = input_ids.shape
        lens = lens.to(dev) if lens is not None else torch.full((B,), S, device=dev,
                                                                dtype=torch.long)
        max_new = max_length or self.max_length
        cfg = self.gpt.cfg
        total = min(int(lens.max().item()) + max_new, cfg.max_position_embeddings)
        p = next(self.parameters())
        attn0 = self.gpt.layers[0].attn
        drafter = self._spec_drafter(B, dev)
        # speculative rounds write spec_tokens rows past the last emitted position
        rows = total + (self.spec_tokens if drafter is not None else 0)
        cache = KVCache(len(self.gpt.layers), B, rows, attn0.heads, attn0.head_dim, p.dtype, dev)
        gen = None
        if seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed)
        cseed = self._coupled_seed(seed, dev)
        # ---- prefill
        logits = self._prompt_logits(input_ids, lens, cache, lens.to(torch.int32))
        eos = self.eos_token_id
        pad = self.pad_token_id if self.pad_token_id is not None else (eos if eos is not None else 0)
        if self.device_loop:
            if topo.mp_world_size() == 1:
                return self._device_loop(input_ids, lens, logits, cache, max_new, pad, gen,
                                         cseed)
            if not self._device_loop_warned:
                warnings.warn("device_loop is ignored under tensor parallelism")
                self._device_loop_warned = True
        if drafter is not None and self.spec_device_loop:
            return self._speculative_device(input_ids, lens, logits, cache, max_new, pad, drafter,
                                            cseed)
        if drafter is not None:
            return self._speculative(input_ids, lens, logits, cache, max_new, pad, total, drafter,
                                     cseed)
        out_tokens, scores, _ = self._host_loop(logits, input_ids.clone(), lens.clone(), cache,
                                                total, max_new, pad, gen, seed=cseed)
        if not out_tokens:
            return torch.zeros(B, 0, dtype=torch.long, device=dev), scores
        return torch.stack(out_tokens, 1), scores

    def _generate_turn(self, s, input_ids, lens, max_length, seed):
        """``generate()`` with a session: see there."""
        tok, count, hcount = self._session_turn(s, input_ids, lens)   # raises before any launch
        self._w8_refresh()
        dev = input_ids.device
        B = s.batch_size
        max_new = max_length or self.max_length
        gen = None
        if seed is not None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(seed)
        cseed = self._coupled_seed(seed, dev)
        start = list(s._lens)
        Sp = tok.shape[1]
        if not any(start) and not (self.prefill_chunk and Sp > self.prefill_chunk):
            # a first turn in one pass: the plain prefill
            logits = self._prompt_logits(tok, count, s.cache, count.to(torch.int32))
        else:
            logits = self._prefill_at(tok, count, start, s.cache)
        s.logits = logits.clone()  # the processors write in place
        s._put(tok, s.lens, count)
        cur = s.lens + count
        end = [a + n for a, n in zip(start, hcount)]
        s.lens.copy_(cur)
        s.pending.fill_(-1)
        s._lens, s._pending = end, [-1] * B
        eos = self.eos_token_id
        pad = self.pad_token_id if self.pad_token_id is not None else (eos if eos is not None else 0)
        total = min(max(end) + max_new, s.max_len)
        out_tokens, scores, emitted = self._host_loop(logits, s.history(), cur.clone(), s.cache,
                                                      total, max_new, pad, gen, count=True,
                                                      seed=cseed)
        if not out_tokens:
            return torch.zeros(B, 0, dtype=torch.long, device=dev), scores
        out = torch.stack(out_tokens, 1)
        # a row that emitted n tokens: n - 1 of them are in the cache, the n-th is pending
        s._put(out, cur, emitted)
        pending = torch.where(emitted > 0,
                              out.gather(1, (emitted - 1).clamp(min=0)[:, None]).squeeze(1),
                              torch.full_like(emitted, -1))
        s.lens.add_((emitted - 1).clamp(min=0))
        s.pending.copy_(pending)
        n = emitted.tolist()
        s._lens = [a + max(k - 1, 0) for a, k in zip(end, n)]
        s._pending = [int(t) for t in pending.tolist()]
        return out, scores

    def _host_loop(self, logits, history, cur, cache, total, max_new, pad, gen, count=False,
                   seed=None):
        """The sampling / greedy loop on the host: ``logits`` [B, V] choose the
        first token, ``history`` [B, L] feeds the processors, ``cur`` [B] is
        the position of the next token, positions stay below ``total``.
        Returns the list of [B] token tensors, the scores [B] and, with
        ``count``, the tokens each row emitted (up to and including its EOS).
        With ``seed`` (``sampler: coupled``) token ``step`` of row ``b`` is the
        coupled pick of index ``(step, b)``."""
        B = logits.shape[0]
        dev = logits.device
        eos = self.eos_token_id
        procs = self._processors(max_new)
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        scores = torch.zeros(B, device=dev)
        emitted = torch.zeros(B, dtype=torch.long, device=dev) if count else None
        out_tokens = []
        graphed = None
        for step in range(max_new):
            if cur.max().item() >= total:
                break
            for pr in procs:
                if hasattr(pr, "cur_len"):
                    pr.cur_len = step
            logits = procs(history, logits)
            if seed is not None:
                nxt, lse = ops.coupled_sample(
                    logits, self.temperature, self.top_k, self.top_p, seed,
                    torch.full((B,), step, dtype=torch.int32, device=dev))
                step_score = logits.gather(1, nxt[:, None]).squeeze(1).float() - lse
            elif self.decode_strategy != "greedy_search" and logits.is_cuda:
                # one fused HIP launch: softmax/T, top-k, top-p, draw, logsumexp
                nxt, lse = ops.fused_sample(logits, self.temperature, self.top_k, self.top_p,
                                            generator=gen)
                step_score = logits.gather(1, nxt[:, None]).squeeze(1).float() - lse
            else:
                logp = torch.log_softmax(logits, -1)
                if self.decode_strategy == "greedy_search":
                    nxt = torch.argmax(logits, -1)
                else:
                    lg = logits / self.temperature if self.temperature not in (None, 1.0) \
                        else logits
                    probs = torch.softmax(lg, -1)
                    if self.top_k:
                        probs = top_k_filter(probs, self.top_k)
                    if self.top_p is not None and self.top_p < 1.0:
                        probs = top_p_filter(probs, self.top_p)
                    nxt = torch.multinomial(probs, 1, generator=gen).squeeze(1)
                step_score = logp.gather(1, nxt[:, None]).squeeze(1)
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            scores = torch.where(unfinished, scores + step_score, scores)
            if count:
                emitted += unfinished
            out_tokens.append(nxt)
            history = torch.cat([history, nxt[:, None]], 1)
            if eos is not None:
                unfinished = unfinished & (nxt != eos)
                if not bool(unfinished.any()):
                    break
            # ---- one decode step (replayed from a HIP graph after the first token)
            if graphed is None and self.use_hip_graph and dev.type == "cuda" \
                    and topo.mp_world_size() == 1:
                graphed = _GraphedDecodeStep(self, cache, B)
            logits = graphed(nxt, cur) if graphed is not None else \
                self._decode_step(nxt, cur, cache)
            cur = cur + 1
        return out_tokens, scores, emitted

    # ---- speculative greedy decoding (spec_draft / set_drafter)
    def _spec_drafter(self, batch, dev):
        """The drafter of this ``generate()`` call, or None for the plain loop:
        no drafter configured, or the window step does not cover the call (then
        the key is ignored with one warning, as ``weight_quant`` is)."""
        self.last_spec_stats = None
        if self._drafter is None and self.spec_draft is None:
            return None
        reason = None
        if topo.mp_world_size() != 1:
            reason = "tensor parallelism"
        elif batch * (self.spec_tokens + 1) > 16:
            reason = "batch * (spec_tokens + 1) = %d rows exceed the 16 of the decode GEMV" \
                % (batch * (self.spec_tokens + 1))
        elif self._drafter is None and (dev.type != "cuda" or not self.fused_decode):
            reason = "the quantised draft needs a GPU and fused_decode"
        if reason is not None:
            if not self._spec_warned:
                warnings.warn("speculative decoding is ignored (%s): the plain loop runs" % reason)
                self._spec_warned = True
            return None
        if self._drafter is not None:
            return self._drafter
        if self._quant_drafter is None:
            self._quant_drafter = _QuantDrafter(self)
        return self._quant_drafter

    def _spec_process(self, logits, hist, valid, step, max_new):
        """The logits processors of ``_processors`` for one window slot, with a
        step index and a history per row: ``hist`` [B, L] with ``valid`` [B, L]
        marking the row's tokens so far, ``step`` [B] the index of the token
        these logits choose.  Forced BOS acts on step 0 only, which the prefill
        logits choose.  Returns a processed copy."""
        lj = logits.clone()
        eos = self.eos_token_id
        if self.min_length and eos is not None:
            lj[:, eos] = torch.where(step < self.min_length, torch.full_like(lj[:, eos], -1e9),
                                     lj[:, eos])
        if self.repetition_penalty and self.repetition_penalty != 1.0:
            # tokens outside the history point at the row's first token (a duplicate
            # index that carries the same value)
            ids = torch.where(valid, hist, hist[:, :1])
            sc = torch.gather(lj, 1, ids)
            sc = torch.where(sc < 0, sc * self.repetition_penalty, sc / self.repetition_penalty)
            lj.scatter_(1, ids, sc)
        if self.forced_eos_token_id is not None:
            f = step == max_new - 1
            lj = torch.where(f[:, None], torch.full_like(lj, -1e9), lj)
            col = lj[:, self.forced_eos_token_id]
            lj[:, self.forced_eos_token_id] = torch.where(f, torch.zeros_like(col), col)
        return lj

    def _speculative(self, input_ids, lens, logits, cache, max_new, pad, total, drafter,
                     seed=None):
        """Greedy search, or with ``seed`` coupled sampling, in rounds of {draft ``spec_tokens`` tokens, verify them
        and one more position in one window step of the target weights, keep
        the longest agreeing prefix plus the target's next token}.  ``logits``
        are the prefill's (they choose token 0).

        Every emitted token is the argmax (the coupled pick of its token index
        and row) of processed target logits, so ids and scores are the target's; the drafter only decides how many window
        steps are run.  Past the first token every cache row is written by a
        window step of ``B * (spec_tokens + 1)`` rows, whose row results do not
        depend on the slot, so the output does not depend on the drafter
        either.  One host read per round (is any row still emitting).

        ``last_spec_stats``: ``rounds``; ``drafted`` = ``spec_tokens * B`` per
        round (finished rows keep their rows and are drafted too);
        ``accepted`` = the leading draft tokens the target agreed with, over
        the rows still emitting (agreement in slots past ``max_dec_len``
        counts, those tokens are not emitted)."""
        dev = input_ids.device
        B, S = input_ids.shape
        eos = self.eos_token_id
        g = self.spec_tokens
        W = g + 1
        T = max(0, total - int(lens.max().item()))  # tokens the plain loop emits without EOS
        stats = {"rounds": 0, "drafted": 0, "accepted": 0}
        self.last_spec_stats = stats
        scores = torch.zeros(B, device=dev)
        if T == 0:
            return torch.zeros(B, 0, dtype=torch.long, device=dev), scores
        # ---- token 0, from the prefill logits, as the plain loop takes it
        procs = self._processors(max_new)
        for pr in procs:
            if hasattr(pr, "cur_len"):
                pr.cur_len = 0
        logits = procs(input_ids, logits)
        rowid = torch.arange(B, dtype=torch.int32, device=dev)

        def choose(x, steps, rows):
            """The picks of the rows of ``x`` [R, V] and their log-probabilities."""
            if seed is None:
                t = torch.argmax(x, -1)
                return t, torch.log_softmax(x, -1).gather(1, t[:, None]).squeeze(1)
            t, lse = ops.coupled_sample(x, self.temperature, self.top_k, self.top_p, seed,
                                        steps, rows)
            return t, x.gather(1, t[:, None]).squeeze(1).float() - lse

        last, scores = choose(logits, torch.zeros_like(rowid), rowid)
        # W slack columns: a row's window may reach past the last emitted token
        out = torch.full((B, T + W), pad, dtype=torch.long, device=dev)
        out[:, 0] = last
        hist = torch.cat([input_ids, out], 1)        # the plain loop's history, per row
        unfinished = torch.ones(B, dtype=torch.bool, device=dev)
        if eos is not None:
            unfinished = last != eos
        emitted = torch.ones(B, dtype=torch.long, device=dev)
        cur = lens.clone()                           # position of `last` (not in the cache yet)
        ar = torch.arange(W, device=dev)
        cols = torch.arange(hist.shape[1], device=dev)[None, :]
        accepted = torch.zeros((), dtype=torch.long, device=dev)
        graphed = None
        if self.use_hip_graph and dev.type == "cuda":
            graphed = _GraphedWindowStep(self, cache, B, W)
        rows = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(W)
        plain_logits = all(isinstance(pr, ForcedBOSTokenLogitsProcessor) for pr in procs)
        pick = None if seed is None else _CoupledPick(self, seed, emitted)
        while True:
            active = unfinished & (emitted < T)
            if not bool(active.any()):
                break
            if pick is not None:
                pick.step = emitted
            d = _propose(drafter, last, cur, cache, g, pick).to(device=dev, dtype=torch.long)
            tok = torch.cat([last[:, None], d], 1).reshape(-1)
            pos = (cur[:, None] + ar[None, :]).reshape(-1)
            before = cur.to(torch.int32)
            lg = graphed(tok, pos, before) if graphed is not None else \
                self._window_step(tok, pos, rows, before, cache)
            lg = lg.view(B, W, -1)
            # slot j chooses token emitted + j from the history plus d_1 .. d_j
            idx = emitted[:, None] + ar[None, :]
            hist.scatter_(1, S + idx[:, :g], d)
            if plain_logits:  # no processor acts past token 0: all slots at once
                t, lp = choose(lg.reshape(B * W, -1), idx.reshape(-1), rowid.repeat_interleave(W))
                t, lp = t.view(B, W), lp.view(B, W)
            else:
                t = torch.empty(B, W, dtype=torch.long, device=dev)
                lp = torch.empty(B, W, device=dev)
                for j in range(W):
                    step = emitted + j
                    lj = self._spec_process(lg[:, j], hist, cols < (S + step)[:, None], step,
                                            max_new)
                    t[:, j], lp[:, j] = choose(lj, step, rowid)
            n = (d == t[:, :g]).long().cumprod(1).sum(1)      # accepted draft tokens
            m = torch.minimum(n + 1, T - emitted)
            emit = (ar[None, :] < m[:, None]) & active[:, None]
            if eos is not None:  # stop at the first EOS inside the accepted window
                hit = emit & (t == eos)
                done = hit.any(1)
                first = torch.where(hit, ar[None, :], W).min(1).values
                m = torch.where(done, first + 1, m)
                emit = (ar[None, :] < m[:, None]) & active[:, None]
                unfinished = unfinished & ~done
            out.scatter_(1, idx, torch.where(emit, t, out.gather(1, idx)))
            hist.scatter_(1, S + idx, torch.where(emit, t, hist.gather(1, S + idx)))
            scores = scores + (lp * emit).sum(1)
            m = torch.where(active, m, torch.zeros_like(m))
            last = torch.where(active, t.gather(1, (m - 1).clamp(min=0)[:, None]).squeeze(1), last)
            emitted = emitted + m
            cur = cur + m
            accepted += (n * active).sum()
            stats["rounds"] += 1
            stats["drafted"] += g * B
        stats["accepted"] = int(accepted.item())
        if hasattr(drafter, "release"):
            drafter.release()
        return out[:, :int(emitted.max().item())], scores

    def _speculative_device(self, input_ids, lens, logits, cache, max_new, pad, drafter,
                            seed=None):
        """``_speculative`` with the verify on the device (``spec_device_loop``):
        token 0 by ``ops.select_token`` on the prefill ``logits``, then rounds
        of ``_GraphedSpecRound`` on a ``SpecState``.  With the built-in drafter
        a round is one graph replay; a ``set_drafter`` drafter is asked from
        the host with the state's device tensors and its tokens are copied
        into ``state.tok`` before the {window step, verify} graph.  The host
        reads ``state.any_active`` every ``spec_poll`` rounds and nothing
        else; a round after every row finished changes no state and writes
        cache rows below ``total + spec_tokens`` only.  At most ``N - 1``
        rounds run (every round of an emitting row emits a token).  Ids,
        scores and ``last_spec_stats`` are those of ``_speculative``."""
        dev = input_ids.device
        B = input_ids.shape[0]
        g = self.spec_tokens
        N = max(0, min(max_new, self.gpt.cfg.max_position_embeddings - int(lens.max().item())))
        self.last_spec_stats = {"rounds": 0, "drafted": 0, "accepted": 0}
        if N == 0:
            return (torch.zeros(B, 0, dtype=torch.long, device=dev), torch.zeros(B, device=dev))
        state = ops.SpecState(
            input_ids, lens, logits.shape[-1], N, g + 1, eos=self.eos_token_id, pad=pad,
            min_len=self.min_length, penalty=self.repetition_penalty,
            forced_bos=self.forced_bos_token_id, forced_eos=self.forced_eos_token_id,
            max_len=max_new, greedy=seed is None, temperature=self.temperature, top_k=self.top_k,
            top_p=self.top_p, seed=seed)
        ops.select_token(logits, state)
        state.start_window()
        pick = None if seed is None else _CoupledPick(self, state.seed, state.step)
        builtin = drafter is self._quant_drafter
        rnd = _GraphedSpecRound(self, cache, state, builtin)
        tok = state.tok.view(B, g + 1)
        for r in range(N - 1):
            if r % self.spec_poll == 0 and not bool(state.any_active.item()):
                break
            if not builtin:
                tok[:, 1:].copy_(_propose(drafter, state.nxt, state.cur, cache, g, pick))
            rnd()
        rounds, accepted, T = torch.stack([state.rounds.max().long(), state.accepted.sum(),
                                           state.finish_len.max().long()]).tolist()
        self.last_spec_stats = {"rounds": rounds, "drafted": g * B * rounds, "accepted": accepted}
        if hasattr(drafter, "release"):
            drafter.release()
        return state.out[:, :T], state.scores

    def _device_loop(self, input_ids, lens, logits, cache, max_new, pad, gen, seed=None):
        """The sampling / greedy loop with the selection on the device
        (``device_loop``): selection 0 on the prefill ``logits``, then up to
        ``N - 1`` times {decode step -> selection}, replayed from one HIP
        graph.  ``N`` is the number of selections the host loop makes (the
        bound of ``_beam_search``).  Replays after the last row finished write
        pads past ``max(finish_len)`` and are trimmed."""
        dev = input_ids.device
        B = input_ids.shape[0]
        eos = self.eos_token_id
        N = max(0, min(max_new, self.gpt.cfg.max_position_embeddings - int(lens.max().item())))
        if N == 0:
            return (torch.zeros(B, 0, dtype=torch.long, device=dev), torch.zeros(B, device=dev))
        greedy = self.decode_strategy == "greedy_search"
        u = None if greedy or seed is not None else torch.rand(N, B, generator=gen, device=dev)
        state = ops.SelectState(
            input_ids, lens, logits.shape[-1], N, greedy=greedy, temperature=self.temperature,
            top_k=self.top_k, top_p=self.top_p, eos=eos, pad=pad, min_len=self.min_length,
            penalty=self.repetition_penalty, forced_bos=self.forced_bos_token_id,
            forced_eos=self.forced_eos_token_id, max_len=max_new, u=u, seed=seed)
        ops.select_token(logits, state)
        step = None
        if self.use_hip_graph and dev.type == "cuda":
            step = _GraphedSelectStep(self, cache, state)
        for t in range(1, N):
            if eos is not None and t % self.eos_poll == 0 \
                    and not bool(state.unfinished.any()):
                break
            if step is not None:
                step()
            else:
                ops.select_token(self._decode_step(state.nxt, state.cur, cache), state)
        T = int(state.finish_len.max().item())
        return state.out[:, :T], state.scores

    def _beam_search(self, input_ids, lens=None, max_length=None):
        """Beam search with ``nb = num_beams`` beams per sample on a
        ``BeamKVCache``.  Returns ``ids [B*num_return_sequences, T]``, best
        first per sample and padded with ``pad``, and the normalised
        ``scores [B*num_return_sequences]``.

        Semantics (the brute-force oracle of tests/test_beam_search_cpu.py
        implements exactly this):

        * the processors (min length, repetition penalty, forced BOS / EOS) act
          on the fp32 logits as in the sampling path, then ``log_softmax``;
          temperature, ``top_k`` and ``top_p`` are ignored;
        * step 0 selects from the single prefill row per sample; later steps
          from ``cand = beam_score[:, None] + logp`` over ``nb*V`` per sample;
        * the top ``2*nb`` candidates are walked highest first, ties towards
          the lower flat ``(beam, token)`` index.  An EOS candidate with rank
          ``< nb`` becomes a finished hypothesis with score
          ``cand / n**length_penalty`` (``n`` = generated tokens including the
          EOS), an EOS candidate with rank ``>= nb`` is dropped, any other
          candidate becomes a running beam until ``nb`` are kept;
        * the pool keeps the best ``nb`` hypotheses per sample (on equal
          scores the earlier one).  A sample is done when its pool is full and
          either ``early_stopping`` is set or the best running beam, normalised
          at the current length, does not beat the pool's worst.  A done sample
          adds nothing more to its pool;
        * at ``max_dec_len``, or at the position limit, the running beams of
          the samples that are not done enter the pool the same way.

        The prefill runs on the B prompts only.  Decode step ``t`` embeds the
        ``B*nb`` chosen tokens at position ``lens[b] + t`` and appends K/V into
        slot ``t``; a reorder gathers ``cache.anc`` and the token history, no
        K/V moves.  Selection and the pool stay in torch, with one host
        synchronisation per step (the termination check, only with an EOS)."""
        dev = input_ids.device
        B, S = input_ids.shape
        nb, nret = self.num_beams, self.num_return_sequences
        lens = lens.to(dev) if lens is not None else torch.full((B,), S, device=dev,
                                                                dtype=torch.long)
        max_new = max_length or self.max_length
        cfg = self.gpt.cfg
        # selection steps, as in the sampling loop: positions stay below the limit
        N = max(0, min(max_new, cfg.max_position_embeddings - int(lens.max().item())))
        if N == 0:
            return (torch.zeros(B * nret, 0, dtype=torch.long, device=dev),
                    torch.zeros(B * nret, device=dev))
        p = next(self.parameters())
        attn0 = self.gpt.layers[0].attn
        G = max(N - 1, 1)
        cache = BeamKVCache(len(self.gpt.layers), B, nb, S, G, attn0.heads, attn0.head_dim,
                            p.dtype, dev)
        cache.plens.copy_(lens)
        # ---- prefill on the B prompts
        logits = self._prompt_logits(input_ids, lens, cache, cache.plens)
        V = logits.shape[-1]
        procs = self._processors(max_new)
        eos = self.eos_token_id
        pad = self.pad_token_id if self.pad_token_id is not None else (eos if eos is not None else 0)
        lp = float(self.length_penalty)
        ninf = float("-inf")
        beam_score = torch.zeros(B, 1, device=dev)
        hist = torch.full((B, nb, N), pad, dtype=torch.long, device=dev)   # generated tokens
        history = input_ids                                                  # prompt + generated
        pool_score = torch.full((B, nb), ninf, device=dev)
        pool_tok = torch.full((B, nb, N), pad, dtype=torch.long, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        slot = torch.zeros(B * nb, dtype=torch.long, device=dev)
        glens = torch.zeros(B, dtype=torch.int32, device=dev)
        rpos = lens.repeat_interleave(nb)
        graphed = None

        def pool_add(score, toks):
            # score [B, nb] (-inf: no entry), toks [B, nb, N]; earlier entries win ties
            both = torch.cat([pool_score, score], 1)
            top, order = torch.sort(both, dim=1, descending=True, stable=True)
            both_tok = torch.cat([pool_tok, toks], 1)
            return top[:, :nb], both_tok.gather(1, order[:, :nb, None].expand(B, nb, N))

        for t in range(N):
            for pr in procs:
                if hasattr(pr, "cur_len"):
                    pr.cur_len = t
            logp = torch.log_softmax(procs(history, logits), -1)
            nrow = logp.shape[0] // B                                        # 1 at step 0
            cand = (beam_score.view(B, nrow, 1) + logp.view(B, nrow, V)).view(B, nrow * V)
            val, flat = _topk_ties_low(cand, 2 * nb)
            parent, tok = flat // V, flat % V
            is_eos = tok == eos if eos is not None else torch.zeros_like(tok, dtype=torch.bool)
            # running beams: the first nb candidates that are not EOS, in order
            keep = torch.sort(is_eos.to(torch.int8), dim=1, stable=True).indices[:, :nb]
            beam_score = val.gather(1, keep)
            parent_k, tok_k = parent.gather(1, keep), tok.gather(1, keep)
            prev = hist if nrow == nb else hist[:, :1]
            if eos is not None:
                # finished hypotheses: EOS candidates of rank < nb (not for done samples)
                fin = is_eos[:, :nb] & ~done[:, None]
                fscore = torch.where(fin, val[:, :nb] / float(t + 1) ** lp,
                                     torch.full_like(val[:, :nb], ninf))
                ftok = prev.gather(1, parent[:, :nb, None].expand(B, nb, N))
                ftok[:, :, t] = tok[:, :nb]
                pool_score, pool_tok = pool_add(fscore, ftok)
            hist = prev.gather(1, parent_k[:, :, None].expand(B, nb, N))
            hist[:, :, t] = tok_k
            if eos is not None:
                full = pool_score[:, -1] > ninf
                best = beam_score[:, 0] / float(t + 1) ** lp
                done = done | (full & (pool_score[:, -1] >= best)) if not self.early_stopping \
                    else done | full
                if bool(done.all()):
                    break
            if t == N - 1:
                break
            # ---- reorder (ancestor table only) and one decode step into slot t
            if nrow == nb:
                cache.reorder(parent_k, t)
            else:
                cache.anc[:, t] = cache._self.repeat(B)
            history = torch.cat([input_ids.repeat_interleave(nb, 0),
                                 hist.view(B * nb, N)[:, :t + 1]], 1)
            slot.fill_(t)
            glens.fill_(t + 1)
            nxt, cur = tok_k.reshape(B * nb), rpos + t
            if graphed is None and self.use_hip_graph and dev.type == "cuda" \
                    and topo.mp_world_size() == 1:
                graphed = _GraphedBeamStep(self, cache, slot, glens)
            logits = graphed(nxt, cur) if graphed is not None else \
                self._beam_decode_step(nxt, cur, cache, slot, glens)
        # ---- the running beams of the samples that are not done enter the pool
        n = t + 1
        fscore = torch.where(done[:, None], torch.full_like(beam_score, ninf),
                             beam_score / float(n) ** lp)
        pool_score, pool_tok = pool_add(fscore, hist)
        ids, scores = pool_tok[:, :nret], pool_score[:, :nret]
        if eos is not None:
            # trim to the longest returned hypothesis (a finished one ends at its EOS)
            has = ids[:, :, :n] == eos
            n = int(torch.where(has.any(-1), has.int().argmax(-1) + 1,
                                torch.full_like(ids[:, :, 0], n)).max().item())
        return ids[:, :, :n].reshape(B * nret, n), scores.reshape(B * nret)

    def forward(self, input_ids, lens=None):
        return self.generate(input_ids, lens)
