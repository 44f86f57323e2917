"""Decode-step sampling cost: fused HIP top-k/top-p kernel vs the PyTorch op
chain (softmax, topk, sort/cumsum/scatter, multinomial, log_softmax).

    python tools/bench_sampling.py [--batch 8 --vocab 50304] [--spec-verify] [--coupled]

``--spec-verify``: GPU time of one ``ops.spec_verify`` (the verify step of a
speculative round: ``spec_pick_kernel`` + ``spec_accept_kernel``) under HIP
graph replay at batch 1 and windows 3 / 5 / 8, next to one ``ops.select_token``
measured the same way.  The state is reset inside the graph so that every
replay does the full work (all drafts accepted).

``--coupled``: one ``ops.coupled_sample`` and one ``ops.select_token`` with the
coupled pick (mode 2) next to the inverse-CDF one (mode 1), at batch 1 under
replay, top-k 50 / top-p 0.75.  ``--spec-verify --coupled``: the windows with
the coupled pick (top-k 50 / top-p 0.75) in place of the greedy one, on the
same logits (the planted token wins the race as well)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch  # noqa: E402


def timeit(fn, iters=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def graph_us(fn, reset, iters=200):
    """GPU microseconds of ``fn`` per graph replay: (reset + fn) minus reset alone."""
    def timed(body):
        body()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        return timeit(g.replay, iters)
    both = timed(lambda: (reset(), fn()))
    return both - timed(reset)


SAMPLER = dict(temperature=1.0, top_k=50, top_p=0.75)


def coupled_bench(V):
    from fleetx_amd import ops
    n_steps = 64
    ids, lens = torch.randint(0, V, (1, 128), device="cuda"), torch.tensor([128], device="cuda")
    lg1 = 3 * torch.randn(1, V, device="cuda")
    seed = torch.tensor([1234], dtype=torch.int64, device="cuda")
    steps = torch.full((1,), 3, dtype=torch.int32, device="cuda")
    line = {"vocab": V, "batch": 1, "top_k": 50, "top_p": 0.75}
    line["coupled_sample_us"] = round(graph_us(
        lambda: ops.coupled_sample(lg1, 1.0, 50, 0.75, seed, steps), lambda: steps.fill_(3)), 1)
    u = torch.rand(n_steps, 1, device="cuda")
    for name, kw in (("select_token_mode1_us", dict(u=u)), ("select_token_mode2_us",
                                                            dict(seed=seed))):
        sel = ops.SelectState(ids, lens, V, n_steps, greedy=False, penalty=1.3, **SAMPLER, **kw)
        line[name] = round(
            graph_us(lambda: ops.select_token(lg1, sel), lambda: sel.step.fill_(3)), 1)
    print(json.dumps(line))


def spec_verify_bench(V, coupled=False):
    from fleetx_amd import ops
    n_steps = 64
    ids, lens = torch.randint(0, V, (1, 128), device="cuda"), torch.tensor([128], device="cuda")
    seed = torch.tensor([1234], dtype=torch.int64, device="cuda")
    kw = dict(greedy=False, seed=seed, **SAMPLER) if coupled else {}
    sel = ops.SelectState(ids, lens, V, n_steps, penalty=1.3, **kw)
    lg1 = torch.randn(1, V, device="cuda")
    line = {"vocab": V, "batch": 1, "coupled": coupled, "select_token_us": round(
        graph_us(lambda: ops.select_token(lg1, sel), lambda: sel.step.fill_(3)), 1)}
    for W in (3, 5, 8):
        st = ops.SpecState(ids, lens, V, n_steps, W, penalty=1.3, **kw)
        lg = torch.randn(W, V, device="cuda")
        slot = torch.arange(W, device="cuda")
        lg[slot, 7 + slot] = 30.0                                   # slot j picks 7 + j ...
        st.tok[1:] = 7 + slot[:-1]                                  # ... and every draft is accepted
        line["spec_verify_w%d_us" % W] = round(
            graph_us(lambda: ops.spec_verify(lg, st), lambda: st.step.fill_(3)), 1)
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--vocab", type=int, default=50304)
    ap.add_argument("--spec-verify", action="store_true")
    ap.add_argument("--coupled", action="store_true")
    a = ap.parse_args()
    if a.spec_verify:
        return spec_verify_bench(a.vocab, a.coupled)
    if a.coupled:
        return coupled_bench(a.vocab)
    from fleetx_amd.ops import fused_sample
    from fleetx_amd.models.language_model.gpt.generation import top_k_filter, top_p_filter
    lg = torch.randn(a.batch, a.vocab, device="cuda") * 3

    def chain():
        logp = torch.log_softmax(lg, -1)
        probs = top_p_filter(top_k_filter(torch.softmax(lg / 0.8, -1), 40), 0.9)
        nxt = torch.multinomial(probs, 1).squeeze(1)
        return logp.gather(1, nxt[:, None])

    def fused():
        nxt, lse = fused_sample(lg, 0.8, 40, 0.9)
        return lg.gather(1, nxt[:, None]).squeeze(1) - lse

    print(json.dumps({"batch": a.batch, "vocab": a.vocab, "torch_chain_us": round(timeit(chain), 1),
                      "fused_us": round(timeit(fused), 1)}))


if __name__ == "__main__":
    main()
