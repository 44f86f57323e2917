"""Decode-attention bandwidth microbenchmark (split-K kernel, csrc/kernels/decode_attn.hip).

Prints one JSON line per case: bytes of K+V cache read / kernel time.  The op
is HBM bound, so the figure of merit is TB/s against the ~8 TB/s peak.

    python tools/bench_decode.py [--dtype bf16|fp16] [--beam-only] [--window-only]

Beam cases (``"op": "beam"``): ``ops.beam_decode_attention`` (prompt stored
once per sample, generated slots through the ancestor table) against
``ops.decode_attention`` on the same contents expanded to B*nb rows, which is
the attention of the design that copies the cache per beam.  The per-step index
copy that design also pays is not included.

Window cases (``"op": "window"``): ``ops.window_decode_attention`` with W
queries per sample against ONE ``ops.decode_attention`` call on the same B and
context.  A speculative round replaces W single-query steps by one window
step, so the figure is how far the window call stays below W single calls.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--beam-only", action="store_true")
    ap.add_argument("--window-only", action="store_true")
    a = ap.parse_args()
    from fleetx_amd import ops
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    for B, H, D, L in () if a.beam_only or a.window_only else ((1, 32, 128, 32768), (8, 32, 128, 4096), (32, 32, 128, 2048),
                       (64, 16, 64, 1024), (4, 32, 128, 16384)):
        q = torch.randn(B, H, D, device="cuda", dtype=dt)
        kc = torch.randn(B, L, H, D, device="cuda", dtype=dt)
        vc = torch.randn(B, L, H, D, device="cuda", dtype=dt)
        lens = torch.full((B,), L, device="cuda", dtype=torch.int32)
        res = {}
        for ns in (1, None):
            for _ in range(3):
                ops.decode_attention(q, kc, vc, lens, nsplit=ns)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                ops.decode_attention(q, kc, vc, lens, nsplit=ns)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.iters
            nbytes = 2 * B * L * H * D * kc.element_size()
            res["split1" if ns == 1 else "auto"] = {"us": round(us, 1),
                                                    "TBps": round(nbytes / us / 1e6, 3)}
        print(json.dumps({"B": B, "H": H, "D": D, "L": L, "dtype": a.dtype,
                          "nsplit_auto": ops.attention.decode_splits(B, H, L), **res}), flush=True)
        del kc, vc
    if not a.window_only:
        beam_cases(a, dt)
    if not a.beam_only:
        window_cases(a, dt)


def _time(fn, iters, reps=20):
    """us per call of ``fn`` with the host out of the way: ``reps`` calls are
    captured into one HIP graph (as the decode step runs in generation) and the
    graph is replayed; at these sizes an eager loop measures the enqueue."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    n = max(1, iters // reps)
    graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (n * reps)


def beam_cases(a, dt):
    from fleetx_amd import ops
    H, D, G = 32, 128, 64
    for B in (1, 2):
        for nb in (4, 8):
            for S in (1024, 4096):
                R = B * nb
                q = torch.randn(R, H, D, device="cuda", dtype=dt)
                kp, vp = (torch.randn(B, S, H, D, device="cuda", dtype=dt) for _ in range(2))
                kg, vg = (torch.randn(R, G, H, D, device="cuda", dtype=dt) for _ in range(2))
                plens = torch.full((B,), S, device="cuda", dtype=torch.int32)
                glens = torch.full((B,), G, device="cuda", dtype=torch.int32)
                anc = torch.randint(0, nb, (R, G), device="cuda").to(torch.int32)
                # the copy design's cache: every row holds prompt + its own ancestors
                rows = (torch.arange(R, device="cuda") // nb * nb)[:, None] + anc.long()
                sl = torch.arange(G, device="cuda")[None, :].expand(R, G)
                kc = torch.cat([kp.repeat_interleave(nb, 0), kg[rows, sl]], 1).contiguous()
                vc = torch.cat([vp.repeat_interleave(nb, 0), vg[rows, sl]], 1).contiguous()
                lens = torch.full((R,), S + G, device="cuda", dtype=torch.int32)
                out = ops.beam_decode_attention(q, kp, vp, plens, kg, vg, glens, anc)
                ref = ops.decode_attention(q, kc, vc, lens)
                err = ((out.float() - ref.float()).norm() / ref.float().norm()).item()
                us_beam = _time(lambda: ops.beam_decode_attention(q, kp, vp, plens, kg, vg,
                                                                  glens, anc), a.iters)
                us_copy = _time(lambda: ops.decode_attention(q, kc, vc, lens), a.iters)
                eb = kp.element_size()
                bytes_beam = 2 * (B * S + R * G) * H * D * eb
                bytes_copy = 2 * R * (S + G) * H * D * eb
                print(json.dumps({
                    "op": "beam", "B": B, "nb": nb, "H": H, "D": D, "prompt": S, "gen": G,
                    "dtype": a.dtype, "rel_diff": round(err, 5),
                    "nsplit_beam": ops.attention.beam_decode_splits(B, H, S + G),
                    "nsplit_expanded": ops.attention.decode_splits(R, H, S + G),
                    "beam": {"us": round(us_beam, 1), "cache_MB": round(bytes_beam / 2**20, 1),
                             "TBps": round(bytes_beam / us_beam / 1e6, 3)},
                    "expanded": {"us": round(us_copy, 1), "cache_MB": round(bytes_copy / 2**20, 1),
                                 "TBps": round(bytes_copy / us_copy / 1e6, 3)},
                    "speedup": round(us_copy / us_beam, 2)}), flush=True)
                del kc, vc


def window_cases(a, dt):
    from fleetx_amd import ops
    H, D = 32, 128
    for B in (1, 2):
        for L in (1024, 4096):
            kc, vc = (torch.randn(B, L + 8, H, D, device="cuda", dtype=dt) for _ in range(2))
            lens1 = torch.full((B,), L, device="cuda", dtype=torch.int32)
            q1 = torch.randn(B, H, D, device="cuda", dtype=dt)
            us_one = _time(lambda: ops.decode_attention(q1, kc, vc, lens1), a.iters)
            for W in (2, 5, 8):
                q = torch.randn(B * W, H, D, device="cuda", dtype=dt)
                lens = torch.full((B,), L - W, device="cuda", dtype=torch.int32)
                out = ops.window_decode_attention(q, kc, vc, lens)
                # the last slot sees L keys: the single-query kernel on the same keys
                ref = ops.decode_attention(q[W - 1::W].contiguous(), kc, vc, lens1)
                err = ((out[W - 1::W].float() - ref.float()).norm() / ref.float().norm()).item()
                us_win = _time(lambda: ops.window_decode_attention(q, kc, vc, lens), a.iters)
                nbytes = 2 * B * L * H * D * kc.element_size()
                print(json.dumps({
                    "op": "window", "B": B, "W": W, "H": H, "D": D, "context": L,
                    "dtype": a.dtype, "rel_diff": round(err, 5),
                    "nsplit_window": ops.attention.window_decode_splits(B, H, L + 8),
                    "nsplit_single": ops.attention.decode_splits(B, H, L + 8),
                    "window": {"us": round(us_win, 1), "TBps": round(nbytes / us_win / 1e6, 3)},
                    "single": {"us": round(us_one, 1), "TBps": round(nbytes / us_one / 1e6, 3)},
                    "window_over_single": round(us_win / us_one, 2),
                    "W_singles_over_window": round(W * us_one / us_win, 2)}), flush=True)
            del kc, vc


if __name__ == "__main__":
    main()
