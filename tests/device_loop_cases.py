"""Shared data for the on-device token selection tests
(test_device_loop_cpu.py, test_device_loop_gpu.py): the single-step cases
against the torch logits processors, and the EOS construction of the
generate-parity tests."""
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt import generation as G

EOS, PAD, BOS = 5, 0, 11
N_STEPS = 8
PEN = 1.3
MIN_LEN = 4

# name -> (step, processor settings).  Every case runs with the repetition
# penalty unless it says otherwise.
CASES = {
    "penalty": dict(step=3),
    "min_len_before": dict(step=MIN_LEN - 1, min_len=MIN_LEN, eos_top=True),
    "min_len_at": dict(step=MIN_LEN, min_len=MIN_LEN, eos_top=True),
    "forced_bos": dict(step=0, forced_bos=BOS),
    "forced_eos": dict(step=N_STEPS - 1, forced_eos=EOS),
    "finished_row": dict(step=3, finished=True),
    "tie": dict(step=2, tie=True, penalty=1.0),
}


def build(name, V, B, device="cpu", greedy=True, sample=None, u=None):
    """The inputs of case ``name``: fp32 ``logits`` [B, V], the ``history``
    [B, 12] (prompt columns plus earlier tokens: duplicates, the pad token and
    EOS in every row, the last vocabulary entry in row 0), a ``SelectState``
    positioned at the case's step, and the case's settings."""
    c = dict(CASES[name])
    g = torch.Generator().manual_seed(1000 + V + B)
    logits = 3.0 * torch.randn(B, V, generator=g)
    hist = torch.randint(0, V, (B, 12), generator=g)
    hist[:, 3] = hist[:, 2]          # a duplicate
    hist[:, 5] = PAD
    hist[:, 6] = EOS
    hist[:, 7] = 7
    hist[:, 8] = 7
    hist[0, 9] = V - 1               # the partial bitmap word
    # penalised logits of both signs in every row
    logits[:, 7] = 2.5
    logits[:, EOS] = -1.5
    if c.get("eos_top"):
        logits[:, EOS] = 40.0        # EOS wins unless the min length masks it
    if c.get("tie"):
        logits[:, V // 3] = 50.0
        logits[:, V - 2] = 50.0
    lens = torch.tensor([9, 4, 7, 9, 6][:B])
    sample = sample or (1.0, 0, 1.0)
    st = ops.SelectState(hist.to(device), lens.to(device), V, N_STEPS, greedy=greedy,
                         temperature=sample[0], top_k=sample[1], top_p=sample[2], eos=EOS, pad=PAD,
                         min_len=c.get("min_len", 0), penalty=c.get("penalty", PEN),
                         forced_bos=c.get("forced_bos"), forced_eos=c.get("forced_eos"), u=u)
    st.step.fill_(c["step"])
    st.scores.copy_(torch.arange(B, dtype=torch.float32) * 0.5)
    if c.get("finished") and B > 1:
        st.unfinished[1] = 0
        st.finish_len[1] = 2
    c["penalty"] = c.get("penalty", PEN)
    return logits.to(device), hist.to(device), st, c


def torch_processed(logits, hist, c):
    """The case's logits after the torch processors, in ``_processors()``' order."""
    procs = G.LogitsProcessorList()
    if c.get("min_len"):
        procs.append(G.MinLengthLogitsProcessor(c["min_len"], EOS))
    if c["penalty"] != 1.0:
        procs.append(G.RepetitionPenaltyLogitsProcessor(c["penalty"]))
    if c.get("forced_bos") is not None:
        procs.append(G.ForcedBOSTokenLogitsProcessor(c["forced_bos"]))
        procs[-1].step = c["step"]
    if c.get("forced_eos") is not None:
        procs.append(G.ForcedEOSTokenLogitsProcessor(N_STEPS, c["forced_eos"]))
    for p in procs:
        if hasattr(p, "cur_len"):
            p.cur_len = c["step"]
    return procs(hist, logits.clone())


def check_step(st, before, x, pick, hist, c, V):
    """After one ``select_token``: every piece of state against the host
    loop's bookkeeping for the pick ``pick`` [B] on processed logits ``x``.
    ``before`` holds (unfinished, scores, finish_len, lens) from before the call."""
    unf0, score0, fin0, lens = [t.cpu() for t in before]
    x, pick = x.cpu().float(), pick.cpu()
    step = c["step"]
    B = x.shape[0]
    unf = unf0 != 0
    tok = torch.where(unf, pick, torch.full_like(pick, PAD))
    assert torch.equal(st.out[:, step].cpu(), tok)
    assert torch.equal(st.nxt.cpu(), tok)
    assert torch.equal(st.cur.cpu(), lens + step)
    assert torch.equal(st.step.cpu(), torch.full((B,), step + 1, dtype=torch.int32))
    fin = unf & (tok == EOS)
    assert torch.equal(st.unfinished.cpu() != 0, unf & ~fin)
    assert torch.equal(st.finish_len.cpu().long(),
                       torch.where(fin, torch.full_like(tok, step + 1), fin0.long()))
    # the bitmap is exactly the history plus this token
    want = torch.zeros(B, V, dtype=torch.bool)
    want.scatter_(1, torch.cat([hist.cpu(), tok[:, None]], 1), True)
    assert torch.equal(ops.sampling.unpack_seen(st.seen.cpu(), V), want)
    assert torch.equal(st.seen.cpu(), ops.sampling._pack_seen(
        torch.cat([hist.cpu(), tok[:, None]], 1), V))
    # per-step score bound (the one on fused_sample's lse)
    lse = torch.logsumexp(x, -1)
    ref = x.gather(1, pick[:, None]).squeeze(1) - lse
    got = st.scores.cpu() - score0
    print("step score err", (got - ref)[unf].abs().max().item() if unf.any() else 0.0)
    assert bool(((got - ref).abs() <= 1e-4 + 1e-5 * lse.abs())[unf].all())
    assert torch.equal(st.scores.cpu()[~unf], score0[~unf])   # a finished row keeps its score
    return tok


def snapshot(st):
    return [t.clone() for t in (st.unfinished, st.scores, st.finish_len, st.lens)]


def varied(model, scale=8.0):
    """A random-init model with tied embeddings repeats one token under greedy
    search; stronger position embeddings make its logits depend on the
    position, so that a run emits many tokens and an EOS can be constructed."""
    with torch.no_grad():
        model.gpt.embeddings.position_embeddings.mul_(scale)
    return model


def pick_eos(ids):
    """A token that the EOS-free run ``ids`` [B, T] emits first at a step in
    3..6 in at least one row and nowhere in steps 0..6 of at least one other."""
    rows = ids.tolist()
    for t in range(3, 7):
        for r in rows:
            tok = r[t]
            first = [row.index(tok) if tok in row[:7] else None for row in rows]
            if any(f is not None and f < 3 for f in first):
                continue
            if any(f is None for f in first):
                return tok
    raise AssertionError("no EOS candidate in %r" % (rows,))


class Spy:
    """Counts, while active, the calls that tell the device loop from the host
    loop: ``ops.select_token`` (through ``generation``'s reference), the
    graphed select step, the host loop's graphed decode step and
    ``ops.fused_sample``.  A ``generate()`` that ignored ``device_loop`` would
    leave ``select`` at 0."""

    def __enter__(self):
        self.select = self.select_graph = self.host_graph = self.fused_sample = 0
        self._saved = (ops.select_token, ops.fused_sample, G._GraphedSelectStep.__call__,
                       G._GraphedDecodeStep.__call__)
        sel, fs, sg, hg = self._saved

        def select_token(*a, **k):
            self.select += 1
            return sel(*a, **k)

        def fused_sample(*a, **k):
            self.fused_sample += 1
            return fs(*a, **k)

        def select_graph(step, *a, **k):
            self.select_graph += 1
            return sg(step, *a, **k)

        def host_graph(step, *a, **k):
            self.host_graph += 1
            return hg(step, *a, **k)
        ops.select_token, ops.fused_sample = select_token, fused_sample
        G._GraphedSelectStep.__call__, G._GraphedDecodeStep.__call__ = select_graph, host_graph
        return self

    def __exit__(self, *exc):
        (ops.select_token, ops.fused_sample, G._GraphedSelectStep.__call__,
         G._GraphedDecodeStep.__call__) = self._saved


def selections(T, N, poll, all_finished):
    """Selections the device loop makes for a result of ``T`` of at most ``N``
    tokens: it stops at the first multiple of ``poll`` at which every row has
    finished, else runs all ``N``."""
    return min(N, -(-T // poll) * poll) if all_finished else N
