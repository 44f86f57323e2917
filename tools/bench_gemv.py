"""Decode GEMV (csrc/kernels/decode_gemv.hip) micro-benchmark: us per call and
weight-stream TB/s for the decoder-layer shapes of GPT 1.3B / 6.7B, against
hipBLASLt (F.linear) on the same operands.  

    python tools/bench_gemv.py [--m 1 8 16]
    python tools/bench_gemv.py --w8 [--m 1 4 16] [--repeat 2]
    python tools/bench_gemv.py --w4 [--m 1 4 16] [--repeat 2]

``--w8`` times the weight-only int8 GEMV (csrc/kernels/decode_gemv_w8.hip)
against the 16-bit one, alternating in one process on weights streamed from
HBM (each series replayed from a HIP graph, so the figure is GPU time); ``--repeat`` runs each series that many times.
``--w4`` does the same for the int4 GEMV with group scales
(csrc/kernels/decode_gemv_w4.hip); its records carry ``gemv_w4_us``."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"1.3B_qkv": (6144, 2048), "1.3B_out": (2048, 2048), "1.3B_fc1": (8192, 2048),
          "1.3B_fc2": (2048, 8192), "6.7B_qkv": (12288, 4096), "6.7B_out": (4096, 4096),
          "6.7B_fc1": (16384, 4096), "6.7B_fc2": (4096, 16384), "lm_head_1.3B": (50304, 2048),
          "lm_head_6.7B": (50304, 4096)}


def timeit(fn, iters=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def time_graph(call, ncopy, iters=20):
    """us per call of ``call(i)`` (i cycles over the weight copies), replayed
    from a captured HIP graph of >= 32 calls: at 5-10 us per kernel an eager
    loop times the Python wrapper, not the GPU."""
    ncall = -(-32 // ncopy) * ncopy
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(ncopy):
            call(i)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(ncall):
            call(i % ncopy)
    return timeit(graph.replay, iters) / ncall


def main_w8(args, G):
    """16-bit against int8 (``--w8``) or int4 (``--w4``) weights."""
    from fleetx_amd import ops
    tag, quantise, gemv, wbytes = ("w4", ops.quantize_weight_int4, G.decode_linear_w4, 0.5) \
        if args.w4 else ("w8", ops.quantize_weight_int8, G.decode_linear_w8, 1.0)
    for name in args.shapes or SHAPES:
        N, K = SHAPES[name]
        # the same count of copies for both (>= 1 GiB of 16-bit, >= 512 MiB of
        # quantised weights: twice the 256 MB Infinity Cache), so every call streams from HBM
        ncopy = max(2, -(-int((1 << 30) // wbytes) // (N * K * 2)))
        ws = [(torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16() for _ in range(ncopy)]
        qs = [quantise(w) for w in ws]
        b = torch.randn(N, device="cuda").bfloat16()
        for M in args.m:
            x = torch.randn(M, K, device="cuda").bfloat16()
            assert gemv(x, qs[0][0], qs[0][1], b) is not None
            us16, us8 = [], []
            for _ in range(args.repeat):
                us16.append(time_graph(lambda i: G.decode_linear(x, ws[i], b), ncopy))
                us8.append(time_graph(lambda i: gemv(x, *qs[i], b), ncopy))
            m16, m8 = min(us16), min(us8)
            print(json.dumps({"shape": name, "M": M, "N": N, "K": K,
                              "gemv16_us": [round(u, 2) for u in us16],
                              "gemv_%s_us" % tag: [round(u, 2) for u in us8],
                              "gemv16_TB_s": round(N * K * 2 / m16 / 1e6, 2),
                              "gemv_%s_TB_s" % tag: round(N * K * wbytes / m8 / 1e6, 2),
                              "speedup": round(m16 / m8, 3),
                              "spread16_pct": round(100 * (max(us16) - m16) / m16, 2)}),
                  flush=True)
        del ws, qs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--warm", action="store_true",
                    help="also time a weight resident in the Infinity Cache")
    ap.add_argument("--w8", action="store_true", help="16-bit vs weight-only int8 GEMV")
    ap.add_argument("--w4", action="store_true", help="16-bit vs weight-only int4 (g256) GEMV")
    ap.add_argument("--repeat", type=int, default=2, help="--w8 / --w4: runs of each series")
    ap.add_argument("--shapes", nargs="+", default=None, choices=sorted(SHAPES))
    args = ap.parse_args()
    from fleetx_amd.ops import gemm as G
    if args.w8 or args.w4:
        return main_w8(args, G)
    for name, (N, K) in SHAPES.items():
        # enough weight copies (>= 1 GiB) that successive calls stream from HBM,
        # as in a decode step over all layers, not from the 256 MB Infinity Cache
        ncopy = max(1, -(-(1 << 30) // (N * K * 2)))
        ws = [(torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16() for _ in range(ncopy)]
        b = torch.randn(N, device="cuda").bfloat16()
        for M in args.m:
            x = torch.randn(M, K, device="cuda").bfloat16()
            it = [0]

            def nxt():
                it[0] = (it[0] + 1) % ncopy
                return ws[it[0]]
            us = timeit(lambda: G.decode_linear(x, nxt(), b))
            ub = timeit(lambda: F.linear(x, nxt(), b))
            rec = {"shape": name, "M": M, "N": N, "K": K,
                   "gemv_us": round(us, 2), "gemv_TB_s": round(N * K * 2 / us / 1e6, 2),
                   "hipblaslt_us": round(ub, 2),
                   "hipblaslt_TB_s": round(N * K * 2 / ub / 1e6, 2)}
            if args.warm:
                # the same weight every call: it stays in the 256 MB Infinity
                # Cache (MALL) -- what a prefetch of the next GEMV's weights
                # under the current phase would buy
                w0 = ws[0]
                uw = timeit(lambda: G.decode_linear(x, w0, b))
                rec.update(gemv_warm_us=round(uw, 2), gemv_warm_TB_s=round(N * K * 2 / uw / 1e6, 2))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
