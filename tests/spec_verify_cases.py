"""Shared data for the on-device speculative verify tests
(test_spec_verify_cpu.py, test_spec_verify_gpu.py): single-call cases of
``ops.spec_verify`` on built logits, and a straightforward per-row Python
reference of one round that uses the torch logits processors."""
import torch

from fleetx_amd import ops
from fleetx_amd.models.language_model.gpt import generation as G

EOS, PAD = 5, 0
N_STEPS = 12
PEN = 1.3
STEP = 3
HIGH = 30.0          # a planted pick: above every other logit, also after the penalty
INT_STATE = ("out", "seen", "step", "cur", "nxt", "unfinished", "finish_len", "tok", "pos",
             "wlens", "rounds", "accepted", "any_active")
ALL_STATE = INT_STATE + ("scores", "picks", "logp")

CASES = ("all_accepted", "none_accepted", "stop_at_2", "eos_accepted", "eos_rejected",
         "draft_penalty", "rejected_absent", "min_len_between", "forced_eos", "truncate",
         "finished_row", "tie", "last_vocab")


def _target(b, j):
    """The token planted as the pick of slot ``j`` of row ``b``: distinct per
    slot, outside the history, not EOS or PAD."""
    return 20 + 3 * j + b


def build(name, V, B, W, device="cpu"):
    """The inputs of case ``name``: fp32 window ``logits`` [B*W, V], the
    ``history`` [B, 12 + step] (prompt columns plus the tokens emitted so far:
    a duplicate, PAD and EOS in every row, the last vocabulary entry in row 0)
    and a ``SpecState`` in the middle of a run, its drafts in ``tok``.  Every
    row plays the case; ``finished_row`` adds rows that no longer emit."""
    g = W - 1
    gen = torch.Generator().manual_seed(7000 + V + 16 * B + W)
    logits = torch.randn(B * W, V, generator=gen)
    lg = logits.view(B, W, V)
    hist = torch.randint(100, V - 1, (B, 12 + N_STEPS), generator=gen)
    hist[:, 3] = hist[:, 2]
    hist[:, 5] = PAD
    hist[:, 6] = EOS
    hist[0, 9] = V - 1
    step, min_len, forced, pen = STEP, 0, None, PEN
    tgt = [[_target(b, j) for j in range(W)] for b in range(B)]
    drafts = [[tgt[b][i] for i in range(g)] for b in range(B)]     # d_{i+1} = pick of slot i
    k = min(2, g)
    if name in ("none_accepted", "rejected_absent", "eos_rejected"):
        for b in range(B):
            drafts[b] = [60 + b + 2 * i for i in range(g)]          # wrong, outside the history
    if name == "stop_at_2" and k < g:
        for b in range(B):
            drafts[b][k] = 70 + b
    if name == "eos_accepted":
        for b in range(B):
            tgt[b][min(1, g)] = EOS
            drafts[b] = [tgt[b][i] for i in range(g)]
    if name == "eos_rejected":
        for b in range(B):
            tgt[b][1] = EOS
    if name == "min_len_between":
        min_len = step + k
        lg[:, :, EOS] = 50.0                                        # EOS wins wherever it may
    if name == "forced_eos":
        forced, step = EOS, N_STEPS - 1 - k                         # forced in slot k
    if name == "truncate":
        step = N_STEPS - k
    if name == "tie":
        pen = 1.0
    for b in range(B):
        for j in range(W):
            lg[b, j, tgt[b][j]] = HIGH
    if name == "draft_penalty":
        # slot 1: A leads B' unless A, which the accepted d_1 puts into the history, is penalised
        for b in range(B):
            a, bp = tgt[b][0], 90 + b
            lg[b, 1, tgt[b][1]] = 0.0
            lg[b, 1, a], lg[b, 1, bp] = 20.0, 18.0
            tgt[b][1] = bp
            if g > 1:
                drafts[b][1] = bp
    if name == "tie":
        lg[:, 0, V // 3] = 50.0
        lg[:, 0, V - 2] = 50.0
    if name == "last_vocab":
        lg[:, 0, V - 1] = HIGH + 2.0                                # 32 / 1.3 < 30 where penalised
    hist = hist[:, :12 + step]                                      # prompt + emitted so far
    lens = torch.tensor([9, 4, 7, 9, 6][:B])
    st = ops.SpecState(hist.to(device), lens.to(device), V, N_STEPS, W, eos=EOS, pad=PAD,
                       min_len=min_len, penalty=pen, forced_eos=forced)
    st.step.fill_(step)
    st.out[:, :step] = hist[:, 12:12 + step].to(device)
    st.nxt.copy_(st.out[:, step - 1])
    st.cur.copy_(st.lens + step - 1)
    st.scores.copy_(torch.arange(B, dtype=torch.float32) * 0.5)
    st.rounds.fill_(2)
    st.accepted.copy_(torch.arange(B, dtype=torch.int32))
    if name == "finished_row":
        st.unfinished[1 if B > 1 else 0] = 0
        st.finish_len[1 if B > 1 else 0] = 2
        if B > 2:
            st.step[2] = N_STEPS                                    # ran out of steps, no EOS
    st.start_window()
    st.tok.view(B, W)[:, 1:] = torch.tensor(drafts, dtype=torch.long).view(B, g).to(device)
    conf = dict(min_len=min_len, penalty=pen, forced_eos=forced)
    return logits.to(device), hist, st, conf


def snapshot(st):
    return {k: getattr(st, k).detach().cpu().clone() for k in ALL_STATE}


def _processed(row, history, conf, step):
    """One slot's logits [V] after the torch processors, in ``_processors()``'
    order, for the token at index ``step`` of a run with ``history``."""
    procs = G.LogitsProcessorList()
    if conf["min_len"]:
        procs.append(G.MinLengthLogitsProcessor(conf["min_len"], EOS))
    if conf["penalty"] != 1.0:
        procs.append(G.RepetitionPenaltyLogitsProcessor(conf["penalty"]))
    if conf["forced_eos"] is not None:
        procs.append(G.ForcedEOSTokenLogitsProcessor(N_STEPS, conf["forced_eos"]))
    for p in procs:
        if hasattr(p, "cur_len"):
            p.cur_len = step
    return procs(history[None], row[None].clone())[0]


def reference(logits, hist, before, conf, V, W):
    """What one ``spec_verify`` must leave, row by row in plain Python from the
    snapshot ``before``: (expected integer state, expected score gain [B], the
    bound on its error [B]: ``1e-4 + 1e-5 |lse|`` per emitted token)."""
    logits = logits.cpu()
    want = {k: v.clone() for k, v in before.items()}
    B = before["step"].shape[0]
    gain, bound = torch.zeros(B), torch.zeros(B)
    emitted = []
    for b in range(B):
        step = int(before["step"][b])
        emitted.append([])
        if not before["unfinished"][b] or step >= N_STEPS:
            continue
        d = before["tok"][b * W + 1:(b + 1) * W].tolist()
        picks, lps, lses = [], [], []
        for j in range(W):
            extra = [t for t in d[:j] if 0 <= t < V]
            h = torch.cat([hist[b], torch.tensor(extra, dtype=torch.long)])
            x = _processed(logits[b * W + j], h, conf, step + j)
            p = int(torch.argmax(x))
            lse = torch.logsumexp(x, -1)
            picks.append(p), lps.append(float(x[p] - lse)), lses.append(float(lse))
        n = 0
        while n < W - 1 and d[n] == picks[n]:
            n += 1
        m = min(n + 1, N_STEPS - step)
        if EOS in picks[:m]:
            m = picks.index(EOS) + 1
            want["unfinished"][b] = 0
            want["finish_len"][b] = step + m
        for j in range(m):
            want["out"][b, step + j] = picks[j]
            gain[b] += lps[j]
            bound[b] += 1e-4 + 1e-5 * abs(lses[j])
        emitted[b] = picks[:m]
        cur = int(before["cur"][b]) + m
        want["nxt"][b] = picks[m - 1]
        want["step"][b] = step + m
        want["cur"][b] = cur
        want["rounds"][b] += 1
        want["accepted"][b] += n
        want["tok"][b * W] = picks[m - 1]
        want["pos"][b * W:(b + 1) * W] = cur + torch.arange(W)
        want["wlens"][b] = cur
    width = max(len(e) for e in emitted)
    # rows that emit less repeat a history token: the set is history + emitted
    full = torch.stack([torch.cat([hist[b], torch.tensor(
        emitted[b] + [int(hist[b, 0])] * (width - len(emitted[b])), dtype=torch.long)])
        for b in range(B)])
    want["seen"] = ops.sampling._pack_seen(full, V)
    want["any_active"][0] = int(((want["unfinished"] != 0) & (want["step"] < N_STEPS)).any())
    return want, gain, bound, emitted


def check(name, got, want, emitted, B, W, V):
    """The named property of case ``name`` on the state ``got`` (a snapshot)."""
    g, k = W - 1, min(2, W - 1)
    n = (got["accepted"] - torch.arange(B, dtype=torch.int32)).tolist()
    m = (got["step"] - STEP).tolist()
    if name == "all_accepted":
        assert n == [g] * B and m == [W] * B
    if name in ("none_accepted", "rejected_absent"):
        assert n == [0] * B and m == [1] * B
    if name == "stop_at_2":
        assert n == [k] * B and m == [k + 1] * B
    if name == "eos_accepted":
        e = min(1, g)
        assert m == [e + 1] * B and not got["unfinished"].any()
        assert got["finish_len"].tolist() == [STEP + e + 1] * B and not got["any_active"][0]
        assert (got["out"][:, STEP + e + 1:] == PAD).all()         # later slots are not emitted
    if name == "eos_rejected":
        assert m == [1] * B and got["unfinished"].all()
    if name == "draft_penalty":
        assert [e[1] for e in emitted] == [90 + b for b in range(B)]
    if name == "min_len_between":
        assert all(e[:k] == [_target(b, j) for j in range(k)] and e[k] == EOS
                   for b, e in enumerate(emitted))
        assert not got["unfinished"].any()
    if name == "forced_eos":
        assert all(e[-1] == EOS and len(e) == k + 1 for e in emitted)
        assert got["finish_len"].tolist() == [N_STEPS] * B
    if name == "truncate":
        assert got["step"].tolist() == [N_STEPS] * B and n == [g] * B
        assert not got["any_active"][0] and got["unfinished"].all()
    if name == "finished_row":
        b = 1 if B > 1 else 0
        assert emitted[b] == [] and got["finish_len"][b] == 2
        assert bool(got["any_active"][0]) == (B > 1)
    if name == "tie":
        assert [e[0] for e in emitted] == [V // 3] * B
    if name == "last_vocab":
        assert emitted[0][0] == _target(0, 0)                       # V - 1 is in row 0's history
        assert all(e[0] == V - 1 for e in emitted[1:])
