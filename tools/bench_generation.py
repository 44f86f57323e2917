"""Decode throughput of GPT generation (greedy, HIP-graph replay) with and
without the fused decode layer (K19: weight-streaming GEMVs with sub-layer
epilogues).  Random-init weights, bf16.

    python tools/bench_generation.py [--model gpt3-1.3B] [--batch 1 8 16] [--tokens 64]
                                     [--strategy beam_search --num-beams 4]
                                     [--weight-quant int8 int4_g256 [--repeat 2]]
                                     [--device-loop [--repeat 3]]
                                     [--spec-draft int4_g256 --spec-tokens 2 4
                                      [--spec-device-loop]]
                                     [--strategy sampling --sampler coupled]

One JSON line per (batch, fused): ms/token, tokens/s and the effective weight
stream rate (parameter bytes / ms per token).  ``--weight-quant int8`` / ``int4_g256`` (or
both) adds the weight-only quantised decode paths to every series, alternating
with the 16-bit one in the same process; ``--repeat`` runs each series that many times (the
spread of the 16-bit repeats is the yardstick for any difference).
``--device-loop`` adds every fused series once more with the token selection
on the device (``Generation.device_loop``), alternating in the same way.
``--spec-draft`` (greedy search) adds one speculative series per ``--spec-tokens``
value on the 16-bit target weights, alternating likewise; its lines report ms
per emitted token, accepted / drafted and the ms of one round (``spec_tokens``
draft steps and one window step), to put another acceptance rate in.
``--spec-device-loop`` adds every speculative series once more with the verify
on the device (``Generation.spec_device_loop``), alternating likewise.
``--sampler coupled`` (with ``--strategy sampling``) draws with the coupled
sampler, under which ``--spec-draft`` applies to sampling as well; every call is
seeded, so the series of one run emit comparable text."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {"gpt-345M": (1024, 24, 16), "gpt3-1.3B": (2048, 24, 16), "gpt3-6.7B": (4096, 32, 32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt3-1.3B", choices=sorted(MODELS))
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--strategy", default="greedy_search",
                    choices=["greedy_search", "sampling", "beam_search"])
    ap.add_argument("--num-beams", type=int, default=1)
    ap.add_argument("--weight-quant", default=[], nargs="+", choices=["int8", "int4_g256"],
                    help="also run the fused decode on weight-only int8 / int4 copies")
    ap.add_argument("--device-loop", action="store_true",
                    help="also run every fused series with Generation.device_loop")
    ap.add_argument("--spec-draft", default=None, choices=["int8", "int4_g256"],
                    help="also run speculative greedy decoding with this draft format")
    ap.add_argument("--spec-tokens", type=int, nargs="+", default=[4])
    ap.add_argument("--sampler", default="inverse_cdf", choices=["inverse_cdf", "coupled"],
                    help="Generation.sampler of a sampling run (top-k 50, top-p 0.75)")
    ap.add_argument("--spec-device-loop", action="store_true",
                    help="also run every speculative series with Generation.spec_device_loop")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--prefill-chunk", type=int, default=0,
                    help="Generation.prefill_chunk for every series; each line then also "
                         "reports the prefill's ms and peak memory")
    ap.add_argument("--session-turns", type=int, default=0,
                    help="instead of the series: a session of --prompt tokens, then this many "
                         "turns of --turn-tokens new tokens, each against prefilling the whole "
                         "transcript again without a session")
    ap.add_argument("--turn-tokens", type=int, default=64)
    ap.add_argument("--max-pos", type=int, default=1024, help="max_position_embeddings")
    args = ap.parse_args()
    from fleetx_amd.models.language_model.gpt.model import GPTConfig, GPTForPretraining
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    h, L, a = MODELS[args.model]
    cfg = GPTConfig(vocab_size=50304, hidden_size=h, num_layers=L, num_attention_heads=a,
                    max_position_embeddings=args.max_pos, hidden_dropout_prob=0.0,
                    attention_probs_dropout_prob=0.0, dtype=torch.bfloat16)
    model = GPTForPretraining(cfg).cuda().eval()
    nbytes = sum(p.numel() * p.element_size() for p in model.parameters())
    if args.session_turns:
        return session_turns(model, args)
    for B in args.batch:
        prompt = torch.randint(0, 50304, (B, args.prompt), device="cuda")
        series = [(f, None, False, 0, False)
                  for f in ((True,) if args.fused_only else (False, True))]
        series += [(True, wq, False, 0, False) for wq in args.weight_quant]
        if args.device_loop and args.strategy != "beam_search":
            series += [(f, wq, True, 0, False) for f, wq, _, _, _ in series if f]
        coupled = args.strategy == "sampling" and args.sampler == "coupled"
        if args.spec_draft and (args.strategy == "greedy_search" or coupled):
            for k in args.spec_tokens:
                series += [(True, None, False, k, sdl)
                           for sdl in ((False, True) if args.spec_device_loop else (False,))]
        for fused, wq, dloop, spec, sdl in series * args.repeat:
            conf = {"max_dec_len": args.tokens, "fused_decode": fused,
                    "decode_strategy": args.strategy, "num_beams": args.num_beams,
                    "weight_quant": wq, "device_loop": dloop,
                    "prefill_chunk": args.prefill_chunk}
            if args.strategy == "sampling":
                conf.update(sampler=args.sampler, top_k=50, top_p=0.75)
            if spec:
                conf.update(spec_draft=args.spec_draft, spec_tokens=spec, spec_device_loop=sdl)
            gen = GPTForGeneration(model, conf)
            seed = {"seed": 1234} if args.strategy == "sampling" else {}
            gen.generate(prompt, max_length=8, **seed)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            gen.generate(prompt, max_length=1, **seed)
            torch.cuda.synchronize()
            t_pre = time.perf_counter() - t0
            peak = torch.cuda.max_memory_allocated() - base
            t0 = time.perf_counter()
            ids, _ = gen.generate(prompt, **seed)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            ms = 1e3 * (t - t_pre) / max(1, ids.shape[1] - 1)
            persistent = fused and B <= 4 and \
                os.environ.get("FLEETX_DECODE_PERSISTENT", "0") == "1"
            line = {"model": args.model, "batch": B, "strategy": args.strategy,
                    "sampler": args.sampler if args.strategy == "sampling" else None,
                    "num_beams": args.num_beams if args.strategy == "beam_search" else 1,
                    "fused_decode": fused, "weight_quant": wq,
                    "device_loop": dloop,
                    "persistent_layers": persistent,
                    "ms_per_token": round(ms, 3),
                    "tokens_per_s": round(B * 1e3 / ms, 1),
                    "weight_TB_s": round(nbytes / (ms * 1e-3) / 1e12, 2)}
            # the max_length=1 call: prefill, one selection, one decode step
            line.update(prefill_chunk=args.prefill_chunk, prefill_ms=round(1e3 * t_pre, 3),
                        prefill_peak_MiB=round(peak / 2 ** 20, 1))
            st = gen.last_spec_stats
            if spec and st:
                # ms_per_token is per emitted token; the weight rate of a 16-bit
                # pass per token does not describe a speculative round
                del line["weight_TB_s"]
                line.update(spec_draft=args.spec_draft, spec_tokens=spec, spec_device_loop=sdl,
                            rounds=st["rounds"],
                            accepted=st["accepted"], drafted=st["drafted"],
                            acceptance=round(st["accepted"] / max(1, st["drafted"]), 3),
                            ms_per_round=round(1e3 * (t - t_pre) / max(1, st["rounds"]), 3))
            print(json.dumps(line), flush=True)


def session_turns(model, args):
    """One JSON line per turn: ms of a turn of ``--turn-tokens`` new tokens on
    the session (prefill of pending + new tokens at the session's offset, one
    selection, one decode step) against the same call on the whole transcript
    without a session; both timed twice, the second one reported."""
    from fleetx_amd.models.language_model.gpt.generation import GPTForGeneration
    conf = {"max_dec_len": args.tokens, "decode_strategy": args.strategy,
            "prefill_chunk": args.prefill_chunk, "eos_token_id": None}
    gen = GPTForGeneration(model, conf)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    for B in args.batch:
        s = gen.new_session(B)
        transcript = torch.randint(0, 50304, (B, args.prompt), device="cuda")
        gen.generate(transcript, max_length=1, session=s)
        for turn in range(args.session_turns):
            new = torch.randint(0, 50304, (B, args.turn_tokens), device="cuda")
            state = (s.lens.clone(), s.pending.clone(), list(s._lens), list(s._pending))
            for rep in range(2):  # the first pass warms the shapes up; state restored between
                s.lens.copy_(state[0])
                s.pending.copy_(state[1])
                s._lens, s._pending = list(state[2]), list(state[3])
                (ids, _), ms_turn = timed(lambda: gen.generate(new, max_length=1, session=s))
            pend = state[1][:, None]
            transcript = torch.cat([transcript, pend, new], 1)
            for rep in range(2):
                _, ms_full = timed(lambda: gen.generate(transcript, max_length=1))
            print(json.dumps({"model": args.model, "batch": B, "turn": turn + 1,
                              "context": int(state[0][0]), "turn_tokens": args.turn_tokens,
                              "prefill_chunk": args.prefill_chunk,
                              "session_turn_ms": round(ms_turn, 3),
                              "full_prefill_ms": round(ms_full, 3),
                              "speedup": round(ms_full / ms_turn, 2)}), flush=True)


if __name__ == "__main__":
    main()
