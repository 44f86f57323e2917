"""Decode GEMV (csrc/kernels/decode_gemv.hip) micro-benchmark: us per call and
weight-stream TB/s for the decoder-layer shapes of GPT 1.3B / 6.7B, against
hipBLASLt (F.linear) on the same operands.  

    python tools/bench_gemv.py [--m 1 8 16]
    python tools/bench_gemv.py --w8 [--m 1 4 16] [--repeat 2]
    python tools/bench_gemv.py --w4 [--m 1 4 16] [--repeat 2]
    python tools/bench_gemv.py --mx4 [--m 1 4 16 32 64] [--repeat 3]
    python tools/bench_gemv.py --rows 17 32 48 64 [--shape nt,ks | --sweep]
    python tools/bench_gemv.py --prefill 65 128 512 2048 [--shape mt,nt | --sweep] [--repeat 3]
    python tools/bench_gemv.py --prefill 65 128 512 2048 --w8a8 [--shape mt,nt,ks | --sweep]

``--w8`` times the weight-only int8 GEMV (csrc/kernels/decode_gemv_w8.hip)
against the 16-bit one, alternating in one process on weights streamed from
HBM (each series replayed from a HIP graph, so the figure is GPU time); ``--repeat`` runs each series that many times.
``--w4`` does the same for the int4 GEMV with group scales
(csrc/kernels/decode_gemv_w4.hip); its records carry ``gemv_w4_us``.
``--mx4`` times the MXFP4 kernels (csrc/kernels/decode_gemv_mx4.hip; above 16
rows GM4 of decode_gemm.hip) against the int4 ones on copies of the same
weights, the two series alternating; its records carry ``w4_us`` / ``mx4_us``.
``--rows`` times the skinny GEMM of 17..64 rows (csrc/kernels/decode_gemm.hip)
in its three formats against the chain it replaces (the vendor GEMM with bias
and the layer's separate GeLU / residual launch), the same way; ``--shape``
pins its launch shape and ``--sweep`` times every shape the library has.
``--prefill`` does the same for the quantised prefill GEMM of 65 rows and more
(csrc/kernels/prefill_gemm.hip; ``--shape mt,nt``), medians of ``--repeat``;
with ``--w8a8`` the W8A8 path (csrc/kernels/prefill_gemm_i8.hip: row quantiser
plus int8 MFMA GEMM, ``--shape mt,nt,ks``) against the weight-only int8 GEMM and
the same chain, with the GEMM alone and its int8 MFMA rate; ``--rounds R`` runs
it as R child processes one after the other, prints the medians over the rounds
and, as the old-versus-old figure, the spread of the two unchanged series (the
chain and the weight-only GEMM, each timed twice per child)."""
import argparse
import json
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"1.3B_qkv": (6144, 2048), "1.3B_out": (2048, 2048), "1.3B_fc1": (8192, 2048),
          "1.3B_fc2": (2048, 8192), "6.7B_qkv": (12288, 4096), "6.7B_out": (4096, 4096),
          "6.7B_fc1": (16384, 4096), "6.7B_fc2": (4096, 16384), "lm_head_1.3B": (50304, 2048),
          "lm_head_6.7B": (50304, 4096), "345M_qkv": (3072, 1024), "345M_out": (1024, 1024),
          "345M_fc1": (4096, 1024), "345M_fc2": (1024, 4096), "lm_head_345M": (50304, 1024)}


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


def main_mx4(args, G):
    """int4 (g256) against MXFP4 weights, GEMV (M <= 16) or skinny GEMM."""
    from fleetx_amd import ops
    for name in args.shapes or SHAPES:
        N, K = SHAPES[name]
        ncopy = max(2, -(-(1 << 31) // (N * K * 2)))   # >= 512 MiB of 4-bit weights
        q4, qm = [], []
        for _ in range(ncopy):
            w = (torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16()
            q4.append(ops.quantize_weight_int4(w))
            qm.append(ops.quantize_weight_mxfp4(w))
        del w
        b = torch.randn(N, device="cuda").bfloat16()
        for M in args.m:
            x = torch.randn(M, K, device="cuda").bfloat16()
            f4, fm = (G.decode_linear_w4, G.decode_linear_mx4) if M <= 16 \
                else (G.decode_gemm_w4, G.decode_gemm_mx4)
            assert f4(x, *q4[0], b) is not None and fm(x, *qm[0], b) is not None
            us4, usm = [], []
            for _ in range(args.repeat):
                us4.append(time_graph(lambda i: f4(x, *q4[i], b), ncopy))
                usm.append(time_graph(lambda i: fm(x, *qm[i], b), ncopy))
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            print(json.dumps({"shape": name, "M": M, "N": N, "K": K,
                              "w4_us": [round(u, 2) for u in us4],
                              "mx4_us": [round(u, 2) for u in usm],
                              "mx4_TB_s": round(N * K * 0.53125 / med(usm) / 1e6, 2),
                              "speedup": round(med(us4) / med(usm), 3),
                              "spread_w4_pct": round(100 * (max(us4) - min(us4)) / min(us4), 2)}),
                  flush=True)
        del q4, qm
        torch.cuda.empty_cache()


def main_rows(args, G):
    """The skinny GEMM at ``--rows`` against the unfused chain of the same call."""
    from fleetx_amd import ops
    pins = [tuple(int(v) for v in args.shape.split(","))] if args.shape else [None]
    if args.sweep:
        pins = [(nt, ks) for nt in (1, 2, 4) for ks in (4, 8)]
    for name in args.shapes or SHAPES:
        N, K = SHAPES[name]
        ncopy = max(2, -(-(1 << 30) // (N * K * 2)))
        ws = [(torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16() for _ in range(ncopy)]
        q8 = [ops.quantize_weight_int8(w) for w in ws]
        q4 = [ops.quantize_weight_int4(w) for w in ws]
        b = torch.randn(N, device="cuda").bfloat16()
        epi = G.GV_GELU if "fc1" in name else G.GV_RES if "out" in name or "fc2" in name \
            else G.GV_BIAS
        for M in args.rows:
            x = torch.randn(M, K, device="cuda").bfloat16()
            res = torch.randn(M, N, device="cuda").bfloat16() if epi == G.GV_RES else None

            def chain(i):
                y = F.linear(x, ws[i], b)
                if epi == G.GV_GELU:
                    y = F.gelu(y, approximate="tanh")
                elif epi == G.GV_RES:
                    y = y + res
                return y
            # every series --repeat times, the series alternating within a repeat
            rec = {"shape": name, "M": M, "N": N, "K": K, "epi": epi, "chain_us": []}
            for _ in range(args.repeat):
                rec["chain_us"].append(round(time_graph(chain, ncopy), 2))
                for pin in pins:
                    kw = dict(epi=epi, res=res, shape=pin)
                    for tag, f in (("w16", lambda i: G.decode_gemm(x, ws[i], b, **kw)),
                                   ("w8", lambda i: G.decode_gemm_w8(x, *q8[i], b, **kw)),
                                   ("w4", lambda i: G.decode_gemm_w4(x, *q4[i], b, **kw))):
                        if f(0) is None:    # not covered, or the rule leaves it to the chain
                            continue
                        key = "%s_%s_us" % (tag, "rule" if pin is None else "%d_%d" % pin)
                        rec.setdefault(key, []).append(round(time_graph(f, ncopy), 2))
            print(json.dumps(rec), flush=True)
        del ws, q8, q4
        torch.cuda.empty_cache()


PREFILL_SHAPES = ["1.3B_qkv", "1.3B_out", "1.3B_fc1", "1.3B_fc2", "6.7B_qkv", "6.7B_out",
                  "6.7B_fc1", "6.7B_fc2", "lm_head_1.3B"]


def main_prefill(args, G):
    """The quantised prefill GEMM (csrc/kernels/prefill_gemm.hip) at ``--prefill``
    rows in its three formats against the prefill's chain on the 16-bit weight
    (the vendor GEMM with bias and the separate GeLU / residual launch), the
    series alternating in one process; medians of ``--repeat`` runs."""
    from fleetx_amd import ops
    pins = [tuple(int(v) for v in args.shape.split(","))] if args.shape else [None]
    if args.sweep:
        pins = [(mt, nt) for mt in (4, 8) for nt in (1, 2, 4)]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for name in args.shapes or PREFILL_SHAPES:
        N, K = SHAPES[name]
        # >= 512 MiB of 4-bit weights (2 GiB of 16-bit ones), as --mx4: the smallest set
        # any series cycles over is twice the 256 MB Infinity Cache, so every call of
        # every series streams from HBM
        ncopy = max(2, -(-(1 << 31) // (N * K * 2)))
        ws = [(torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16() for _ in range(ncopy)]
        qs = {"w8": ([ops.quantize_weight_int8(w) for w in ws], G.prefill_gemm_w8),
              "w4": ([ops.quantize_weight_int4(w) for w in ws], G.prefill_gemm_w4),
              "mx4": ([ops.quantize_weight_mxfp4(w) for w in ws], G.prefill_gemm_mx4)}
        b = torch.randn(N, device="cuda").bfloat16()
        epi = G.GV_GELU if "fc1" in name else G.GV_RES if "out" in name or "fc2" in name \
            else G.GV_BIAS
        for M in args.prefill:
            x = torch.randn(M, K, device="cuda").bfloat16()
            res = torch.randn(M, N, device="cuda").bfloat16() if epi == G.GV_RES else None

            def chain(i):
                y = F.linear(x, ws[i], b)
                if epi == G.GV_GELU:
                    y = F.gelu(y, approximate="tanh")
                elif epi == G.GV_RES:
                    y = y + res
                return y
            runs = {"chain_us": []}
            for _ in range(args.repeat):
                runs["chain_us"].append(time_graph(chain, ncopy, iters=5))
                for pin in pins:
                    for tag, (q, f) in qs.items():
                        call = lambda i: f(x, *q[i], b, epi, res=res, shape=pin)  # noqa: E731
                        if call(0) is None:
                            continue
                        key = "%s_%s_us" % (tag, "rule" if pin is None else "%d_%d" % pin)
                        runs.setdefault(key, []).append(time_graph(call, ncopy, iters=5))
            rec = {"shape": name, "M": M, "N": N, "K": K, "epi": epi}
            rec.update({k: round(med(v), 1) for k, v in runs.items()})
            print(json.dumps(rec), flush=True)
        del ws, qs
        torch.cuda.empty_cache()


def main_prefill_i8(args, G):
    """Quantise + W8A8 GEMM (``q_*``), the GEMM alone on rows quantised once
    (``g_*``), the weight-only int8 GEMM (``w8_rule_us``) and the 16-bit chain,
    the series alternating in one process; medians of ``--repeat`` runs."""
    from fleetx_amd import ops
    pins = [tuple(int(v) for v in args.shape.split(","))] if args.shape else [None]
    if args.sweep:
        pins = [(mt, nt, ks) for mt in (4, 8) for nt in (1, 2, 4) for ks in (1, 2, 4)]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for name in args.shapes or PREFILL_SHAPES:
        N, K = SHAPES[name]
        ncopy = max(2, -(-(1 << 30) // (N * K)))   # >= 1 GiB of int8: every call streams from HBM
        ws = [(torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16() for _ in range(ncopy)]
        q = [ops.quantize_weight_int8(w) for w in ws]
        b = torch.randn(N, device="cuda").bfloat16()
        epi = G.GV_GELU if "fc1" in name else G.GV_RES if "out" in name or "fc2" in name \
            else G.GV_BIAS
        for M in args.prefill:
            x = torch.randn(M, K, device="cuda").bfloat16()
            xq, sx = ops.quantize_rows_int8(x)
            res = torch.randn(M, N, device="cuda").bfloat16() if epi == G.GV_RES else None

            def chain(i):
                y = F.linear(x, ws[i], b)
                if epi == G.GV_GELU:
                    y = F.gelu(y, approximate="tanh")
                elif epi == G.GV_RES:
                    y = y + res
                return y
            runs = {"chain_us": [], "w8_rule_us": [], "quant_us": []}
            w8 = lambda i: G.prefill_gemm_w8(x, *q[i], b, epi, res=res)  # noqa: E731
            for _ in range(args.repeat):
                runs["chain_us"].append(time_graph(chain, ncopy, iters=5))
                runs["w8_rule_us"].append(time_graph(w8, ncopy, iters=5))
                runs["quant_us"].append(time_graph(lambda i: ops.quantize_rows_int8(x), ncopy,
                                                   iters=5))
                for pin in pins:
                    kw = dict(res=res, shape=pin)
                    tag = "rule" if pin is None else "%d_%d_%d" % pin
                    runs.setdefault("q_%s_us" % tag, []).append(time_graph(
                        lambda i: G.prefill_gemm_w8a8(*ops.quantize_rows_int8(x), *q[i], b, epi,
                                                      **kw), ncopy, iters=5))
                    runs.setdefault("g_%s_us" % tag, []).append(time_graph(
                        lambda i: G.prefill_gemm_w8a8(xq, sx, *q[i], b, epi, **kw), ncopy,
                        iters=5))
                # the two unchanged series once more, after everything else: old versus old
                runs.setdefault("chain_again_us", []).append(time_graph(chain, ncopy, iters=5))
                runs.setdefault("w8_again_us", []).append(time_graph(w8, ncopy, iters=5))
            rec = {"shape": name, "M": M, "N": N, "K": K, "epi": epi}
            rec.update({k: round(med(v), 1) for k, v in runs.items()})
            best = min(v for k, v in rec.items() if k.startswith("g_"))
            rec["gemm_int8_TOPS"] = round(2.0 * M * N * K / best / 1e6, 1)
            print(json.dumps(rec), flush=True)
        del ws, q
        torch.cuda.empty_cache()


def rounds_prefill_i8(args):
    """``--w8a8 --rounds R``: R child processes of the same command, one after
    the other (a failed child ends the run); per case the medians over the
    rounds and ``old_spread_pct``, (max - min) / min over the 2 R samples of
    each unchanged series, the larger of the two."""
    cmd = [sys.executable, os.path.abspath(__file__)] + [a for a in sys.argv[1:]]
    i = cmd.index("--rounds")
    del cmd[i:i + 2]
    got = {}
    for _ in range(args.rounds):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("child failed (%d):\n%s" % (r.returncode, r.stderr[-3000:]))
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                rec = json.loads(ln)
                got.setdefault((rec["shape"], rec["M"]), []).append(rec)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for recs in got.values():
        out = {k: recs[0][k] for k in ("shape", "M", "N", "K", "epi")}
        for k in recs[0]:
            if k.endswith("_us"):
                out[k] = med([r[k] for r in recs])
        spread = []
        for a, b in (("chain_us", "chain_again_us"), ("w8_rule_us", "w8_again_us")):
            v = [r[a] for r in recs] + [r[b] for r in recs]
            spread.append(100.0 * (max(v) - min(v)) / min(v))
        out["old_spread_pct"] = round(max(spread), 1)
        out["gemm_int8_TOPS"] = round(2.0 * out["M"] * out["N"] * out["K"] / min(
            v for k, v in out.items() if k.startswith("g_")) / 1e6, 1)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=0,
                    help="--w8a8: run as this many child processes, print medians and spread")
    ap.add_argument("--w8a8", action="store_true",
                    help="--prefill: time the W8A8 path (--shape mt,nt,ks; --sweep: every one)")
    ap.add_argument("--prefill", type=int, nargs="+", default=None,
                    help="time the quantised prefill GEMM at these row counts (>= 65); "
                         "--shape mt,nt pins its launch shape, --sweep times every one")
    ap.add_argument("--m", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--warm", action="store_true",
                    help="also time a weight resident in the Infinity Cache")
    ap.add_argument("--w8", action="store_true", help="16-bit vs weight-only int8 GEMV")
    ap.add_argument("--w4", action="store_true", help="16-bit vs weight-only int4 (g256) GEMV")
    ap.add_argument("--mx4", action="store_true", help="int4 (g256) vs MXFP4 GEMV / skinny GEMM")
    ap.add_argument("--repeat", type=int, default=2,
                    help="--w8 / --w4 / --mx4: runs of each series")
    ap.add_argument("--shapes", nargs="+", default=None, choices=sorted(SHAPES))
    ap.add_argument("--rows", type=int, nargs="+", default=None,
                    help="time the 17..64-row skinny GEMM at these row counts")
    ap.add_argument("--shape", default=None, help="--rows: pin the launch shape, nt,ks")
    ap.add_argument("--sweep", action="store_true", help="--rows: every launch shape")
    args = ap.parse_args()
    if args.prefill and args.w8a8 and args.rounds:
        return rounds_prefill_i8(args)
    from fleetx_amd.ops import gemm as G
    if args.prefill and args.w8a8:
        return main_prefill_i8(args, G)
    if args.prefill:
        return main_prefill(args, G)
    if args.rows:
        return main_rows(args, G)
    if args.mx4:
        return main_mx4(args, G)
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
