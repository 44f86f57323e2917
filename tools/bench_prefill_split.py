"""The sweep behind ``ops.attention.prefill_splits`` on the MI355X
(profiles/prefill_split/README.md): one ``prefill_attention`` call of ROWS
queries at the end of a context, per ``nsplit``, timed by
``bench_attention.turn_times``.

The driver starts one child process per (round, library, dtype), the variants
alternating inside a round, and prints one markdown row per case: the median
over the rounds per ``nsplit``, and for ``nsplit`` 1 (timed first and last in
every child) the median with (min - max) of all its samples, the noise figure.

    python tools/bench_prefill_split.py [--rounds 3] [--h 32] [--b 1 2 8]
        [--lib build/lab/_kernels_x.so ...]     # lab builds next to the default
"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
NS = [1, 2, 4, 8, 16, 0]  # 0: the rule


def child(a):
    import torch
    import bench_attention as BA
    from fleetx_amd import ops
    dt = torch.bfloat16 if a.child == "bf16" else torch.float16
    for H in a.h:
        for B in a.b:
            for S in a.s:
                for rows in a.rows:
                    t = BA.turn_times(ops, B, S, H, a.d, dt, rows, NS, a.iters)
                    t["1b"] = BA.turn_times(ops, B, S, H, a.d, dt, rows, [1], a.iters)[1]
                    print(json.dumps({"dtype": a.child, "H": H, "B": B, "S": S, "rows": rows,
                                      "auto": t.pop("auto"),
                                      "ms": {str(k): v for k, v in t.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, nargs="+", default=[32])
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--b", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--s", type=int, nargs="+", default=[1024, 2048, 4096, 8192])
    ap.add_argument("--rows", type=int, nargs="+", default=[65, 128, 512])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp16"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", nargs="*", default=[], help="FLEETX_KERNELS_LIB builds to alternate "
                    "with the default library")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    got = collections.defaultdict(list)
    for _ in range(a.rounds):
        for lib in [""] + a.lib:
            for dtype in a.dtypes:
                env = dict(os.environ)
                if lib:
                    env["FLEETX_KERNELS_LIB"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", dtype]
                                   + [x for x in sys.argv[1:]], env=env, capture_output=True,
                                   text=True, timeout=600)
                if r.returncode != 0:  # a failed child ends the sweep: nothing more is started
                    raise SystemExit("child failed (%d):\n%s" % (r.returncode, r.stderr[-3000:]))
                for line in r.stdout.splitlines():
                    if line.startswith("{"):
                        c = json.loads(line)
                        key = (os.path.basename(lib) or "default", c["dtype"], c["H"], c["B"],
                               c["S"], c["rows"], c["auto"])
                        got[key].append(c["ms"])
    med = statistics.median
    print("| library | dtype | H | B | context | rows | nsplit 1 (min - max) | 2 | 4 | 8 | 16 | rule "
          "| rule ms | rule wins by more than the spread |")
    print("|" + "---|" * 14)
    for key in sorted(got):
        ms = got[key]
        base = [m["1"] for m in ms] + [m["1b"] for m in ms]
        b, rule = med(base), med([m["0"] for m in ms])
        win = "-" if key[6] == 1 else ("yes" if rule < b - (max(base) - min(base)) else "NO")
        print("| %s | %s | %d | %d | %d | %d | %.4f (%.4f - %.4f) | %s | %d | %.4f | %s |" % (
            key[:6] + (b, min(base), max(base),
                       " | ".join("%.4f" % med([m[n] for m in ms]) for n in ("2", "4", "8", "16")),
                       key[6], rule, win)))


if __name__ == "__main__":
    main()
