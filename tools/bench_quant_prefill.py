"""End-to-end cost of ``Generation.weight_quant_prefill`` on the MI355X
(profiles/quant_prefill/README.md): GPT 1.3B (random weights), batch 1, the
one-pass prefill of a 512- and a 2048-token prompt and a 65-token session turn
over 2048 cached keys, with the key on against the key off (the 16-bit prefill).

The driver starts one child process per (round, format, key), on and off
alternating, and prints one markdown row per (format, case): the medians over
the rounds and the ratio on / off.

    python tools/bench_quant_prefill.py [--rounds 3] [--quant int8 int4_g256 mxfp4]
    python tools/bench_quant_prefill.py --quant int8 --act

``--act`` adds a third child per round, ``Generation.prefill_act_quant: int8``
on top of the key (int8 only), and its columns.
"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ["prompt 512", "prompt 2048", "turn 65 over 2048"]


def child(a):
    import torch
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    from fleetx_amd.models.language_model.gpt import generation as G
    torch.manual_seed(0)
    cfg = GPTConfig(vocab_size=50304, hidden_size=2048, num_layers=24, num_attention_heads=16,
                    max_position_embeddings=4096, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    model = GPTForPretraining(cfg).cuda().eval()
    conf = {"weight_quant": a.child, "weight_quant_prefill": a.key != "off"}
    if a.key == "act":
        conf["prefill_act_quant"] = "int8"
    gen = G.GPTForGeneration(model, conf).eval()
    assert gen.requantize() is True
    dev = "cuda"

    def timed(fn):
        for _ in range(2):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.iters

    def cache(rows):
        return G.KVCache(cfg.num_layers, 1, rows, 16, 128, torch.bfloat16, dev)
    ms = {}
    with torch.no_grad():
        for S in (512, 2048):
            ids = torch.randint(0, 50304, (1, S), device=dev)
            lens, c = torch.tensor([S], device=dev), cache(S)
            ms["prompt %d" % S] = timed(lambda: gen._prompt_logits(ids, lens, c, lens.int()))
        tok, cnt, c = torch.randint(0, 50304, (1, 65), device=dev), torch.tensor([65], device=dev), \
            cache(2048 + 65)
        ms[CASES[2]] = timed(lambda: gen._prefill_at(tok, cnt, [2048], c))
    print(json.dumps({"quant": a.child, "key": a.key, "ms": ms}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quant", nargs="+", default=["int8", "int4_g256", "mxfp4"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--act", action="store_true",
                    help="also time prefill_act_quant: int8 on top of the key (int8 only)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--key", default="off", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    got = collections.defaultdict(list)
    for _ in range(a.rounds):
        for quant in a.quant:
            for key in ("off", "on") + (("act",) if a.act and quant == "int8" else ()):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", quant,
                                    "--key", key, "--iters", str(a.iters)], capture_output=True,
                                   text=True, timeout=300)
                if r.returncode != 0:  # a failed child ends the run: nothing more is started
                    raise SystemExit("child failed (%d):\n%s" % (r.returncode, r.stderr[-3000:]))
                c = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                print(json.dumps(c), file=sys.stderr, flush=True)  # progress
                for case, v in c["ms"].items():
                    got[(quant, case, key)].append(v)
    print("| format | case | key off ms (min - max) | key on ms (min - max) | on / off |")
    print("|---|---|---|---|---|")
    for quant in a.quant:
        for case in CASES:
            off, on = got[(quant, case, "off")], got[(quant, case, "on")]
            mo, mn = statistics.median(off), statistics.median(on)
            print("| %s | %s | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.2f |" % (
                quant, case, mo, min(off), max(off), mn, min(on), max(on), mn / mo))
            act = got.get((quant, case, "act"))
            if act:
                ma = statistics.median(act)
                print("| %s + act int8 | %s | | %.2f (%.2f - %.2f) | %.2f |" % (
                    quant, case, ma, min(act), max(act), ma / mo))


if __name__ == "__main__":
    main()
