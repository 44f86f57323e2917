"""Headline benchmark: GPT-3 6.7B pretraining tokens/s (whole job) on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N>1
it is launched by ``torch.distributed.run`` (one rank per GPU, RCCL).  W
untimed warmup steps, then exactly K full training steps (forward, backward,
gradient reduction, global-norm clip, AdamW update, LR step) bracketed by a
barrier + device synchronize; the elapsed time is the MAX over ranks; rank 0
prints one JSON line.

Config = BASELINE.json metric "tokens/sec (whole node) GPT-3 6.7B
hybrid-parallel at 1/2/4/8 MI355X": h 4096, 32 layers, 32 heads, vocab
50304, seq 1024, dropout 0.1 (as ``pretrain_gpt_6.7B_sharding16.yaml``), bf16
compute with fp32 master weights, synthetic tokens, random-init weights.
Layouts: BASELINE.json config 3's hybrid family by default on N > 1 GPUs --
N=8: TP2 x PP2 x DP2 (1F1B, micro-batch 4, 8 micro-batches per step),
N=4: TP2 x PP2, N=2: TP2 -- so the scaling curve runs tensor- and
pipeline-parallel traffic over RCCL/xGMI, not only data parallel; one GPU
runs the planner's choice (micro-batch 8, no recompute for 6.7B).
``--layout planner`` asks the MI355X layout planner on N > 1 too
(``fleetx_amd/parallel/auto/planner.py``: step-time model with per-link xGMI
bandwidth, 1F1B bubble, ZeRO traffic and the 288 GB budget), and
``--layout dp,mp,pp,micro[,sharding[,stage]]`` pins one.  The JSON line's
``config.parallelism`` names the layout.  Weak scaling: 8 sequences x 1024
tokens of work per GPU per step.  On one GPU the step is captured as one HIP
graph during the warmup (``--hip-graph``; needs ``--warmup >= 3``) and
replayed for the K timed steps, each replay a full step with fresh dropout
masks and the scheduler's learning rate.

A plain run does only what the headline figure needs: setup, warmup, the K
timed steps, the result line.  ``--dump-outputs DIR`` adds, after the timed
steps, ``DIR/loss.npy`` and ``DIR/params_sample.npy`` (the last step's loss and
a seeded sample of the parameters it updated; tokens, initial weights and
dropout salts are seeded, so two builds can be compared output for output).
``--full`` is where measurements beyond the headline figure belong; there are
none today, so it changes nothing yet.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# Multi-rank: one HIP hardware queue per peer-waiting stream (compute + one per
# RCCL communicator), set before the HIP runtime initialises
# (fleetx_amd/utils/streams.py; the pool allows up to 32).
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    from fleetx_amd.utils.streams import ensure_hw_queues  # noqa: E402
    ensure_hw_queues(8)

MODELS = {
    # name: (hidden, layers, heads)
    "gpt3-6.7B": (4096, 32, 32),
    "gpt3-1.3B": (2048, 24, 16),
    "gpt-345M": (1024, 24, 16),
    "gpt-tiny": (256, 2, 4),
    # GPT-3 175B layer shapes (h 12288, 96 heads) with 4 layers: the kernels of
    # BASELINE config 4 measured on one GPU (the full model needs 16 nodes:
    # configs/nlp/gpt/pretrain_gpt_175B_tp8_sharding16_stage3.yaml)
    "gpt3-175B-4L": (12288, 4, 96),
}
from fleetx_amd.utils.hw import PEAK_DENSE_FLOPS  # noqa: E402
PEAK_BF16 = PEAK_DENSE_FLOPS["bfloat16"]  # MI355X dense bf16 (spec), per GPU
# Reference (V100) throughput per GPU on the same model/batch/seq:
# row 1 (345M single card, 16.2k tokens/s) and row 4 (1.3B dp8, ~3.3k tokens/s/GPU,
# derived).  The 6.7B headline config has no published reference number.
REF_TOKENS_PER_GPU = {"gpt-345M": 16200.0, "gpt3-1.3B": 3300.0}
# BASELINE.json config 3 ("GPT-3 6.7B TP=2 PP=2 DP=2 on 8 x MI355X, 1F1B +
# RCCL") and its sub-node members: dp,mp,pp,micro (per-GPU work fixed)
CONFIG3_FAMILY = {2: "1,2,1,8", 4: "1,2,2,4", 8: "2,2,2,4"}



def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="gpt3-6.7B", choices=sorted(MODELS))
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--per-gpu-seqs", type=int, default=8,
                    help="sequences of work per GPU per step (weak scaling)")
    ap.add_argument("--layout", default=None,
                    help="'planner', or dp,mp,pp,micro[,sharding[,stage]], e.g. 2,2,2,4 "
                         "(default: BASELINE config-3 family for gpt3-6.7B, planner otherwise)")
    ap.add_argument("--recompute", action="store_true")
    ap.add_argument("--sequence-parallel", action="store_true")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--grad-reduce-dtype", default=None, choices=["float32", "bfloat16"],
                    help="gradient reduction wire dtype (default: bf16 when N > 1)")
    ap.add_argument("--hip-graph", type=int, default=-1,
                    help="capture the whole step in one HIP graph (1/0; default: on for one "
                         "GPU when --warmup >= 3 covers the capture; the forward-overlapped "
                         "AdamW then runs deferred inside the captured step)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last one computed as "
                         "DIR/<name>.npy: loss.npy (the loss the step returned) and "
                         "params_sample.npy (a fixed seeded sample of every parameter it "
                         "updated); with the same arguments the inputs repeat run to run")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline figure (none today: "
                         "a plain run already does only setup, warmup, the timed steps and "
                         "the result line; new side measurements go behind this flag)")
    return ap.parse_args()


# --dump-outputs: elements sampled per parameter tensor (fp32: a 6.7B model's
# ~390 tensors come to ~6 MB, far under the 64 MB a dump may take)
DUMP_SAMPLE = 4096


def dump_outputs(path, engine, module, lval, write=True):
    """Write the last timed step's results for an output-for-output comparison
    of two builds: the loss it returned and a seeded sample of the parameters
    it left behind (a deferred AdamW is applied first).  Rank 0 writes its own
    shard; the sample indices depend only on each tensor's position and size."""
    import numpy as np
    import torch
    engine._flush_deferred_update()  # every rank: a ZeRO update gathers
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if not write:
        return
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "loss.npy"), np.asarray([lval], dtype=np.float64))
    parts = []
    with torch.no_grad():
        for i, (_, p) in enumerate(module.model.named_parameters()):
            flat = p.detach().reshape(-1)
            if flat.numel() > DUMP_SAMPLE:
                g = torch.Generator()
                g.manual_seed(977 + i)
                idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE,), generator=g)
                flat = flat[idx.to(flat.device)]
            parts.append(flat.float().cpu())
    np.save(os.path.join(path, "params_sample.npy"), torch.cat(parts).numpy())


# the engine captures the step after this many eager steps
# (EagerEngine._fit_graphed(warmup=2)): the capture is the step after them
GRAPH_EAGER_STEPS = 2


def use_graph(flag, n, warmup):
    """Whole-step HIP graph on one GPU (profiles/r4_g67: 6.7B -0.3 to -2.9 ms,
    1.3B -1.3 ms, 345M as before), only when the warmup covers the capture
    step so it never lands inside the timed region; ``flag`` >= 0 forces it."""
    if flag >= 0:
        return int(flag)
    return int(n == 1 and warmup >= GRAPH_EAGER_STEPS + 1)


def main():
    args = parse()
    import torch
    import torch.distributed as dist
    from fleetx_amd.utils import config as cfgmod
    from fleetx_amd.utils import env
    from fleetx_amd.models import build_module
    from fleetx_amd.core.engine.eager_engine import EagerEngine
    from fleetx_amd.models.language_model.gpt.model import flops_per_token
    from fleetx_amd.utils.log import logger

    world = int(os.environ.get("WORLD_SIZE", "1"))
    n = world
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            print("bench.py --gpus %d must be launched with torch.distributed.run" % args.gpus,
                  file=sys.stderr)
            sys.exit(2)
    h, L, a = MODELS[args.model]
    global_batch = args.per_gpu_seqs * n
    recompute = bool(args.recompute)
    sharding, stage = 1, 1
    layout = args.layout
    if layout is None and n > 1:
        layout = CONFIG3_FAMILY.get(n)
    if layout and layout != "planner":
        vals = [int(x) for x in layout.split(",")]
        dp, mp, pp, micro = vals[:4]
        sharding = vals[4] if len(vals) > 4 else 1
        stage = vals[5] if len(vals) > 5 else 1
    else:
        from fleetx_amd.parallel.auto.planner import plan
        p = plan(h, L, a, 50304, args.seq, global_batch, n)
        dp, mp, pp, micro, sharding = p.dp, p.mp, p.pp, p.micro_batch, p.sharding
        stage = max(1, p.sharding_stage)
        recompute = recompute or p.recompute
    assert dp * mp * pp * sharding == n, "layout {} does not match {} GPUs".format(
        (dp, mp, pp, sharding), n)
    local_batch = global_batch // (dp * sharding)
    micro = min(micro, local_batch)
    drop = 0.0 if args.no_dropout else 0.1
    here = os.path.dirname(os.path.abspath(__file__))
    cfg_file = os.path.join(here, "fleetx_amd/configs/nlp/gpt/pretrain_gpt_345M_single_card.yaml")
    ov = ["Model.hidden_size=%d" % h, "Model.num_layers=%d" % L,
          "Model.num_attention_heads=%d" % a, "Model.vocab_size=50304",
          "Model.hidden_dropout_prob=%s" % drop, "Model.attention_probs_dropout_prob=%s" % drop,
          "Model.max_position_embeddings=%d" % max(1024, args.seq),
          "Model.use_recompute=%s" % recompute,
          "Model.sequence_parallel=%s" % bool(args.sequence_parallel),
          "Global.local_batch_size=%d" % local_batch, "Global.micro_batch_size=%d" % micro,
          "Global.global_batch_size=None",
          "Distributed.dp_degree=%d" % dp, "Distributed.mp_degree=%d" % mp,
          "Distributed.pp_degree=%d" % pp,
          "Distributed.sharding.sharding_degree=%d" % sharding,
          "Distributed.sharding.sharding_stage=%d" % stage,
          "Engine.max_steps=%d" % (args.steps + args.warmup), "Engine.logging_freq=1000000",
          "Engine.save_load.save_steps=-1", "Engine.mix_precision.dtype=bfloat16",
          "Data.Train.dataset.max_seq_len=%d" % args.seq,
          "Data.Train.dataset.name=SyntheticGPTDataset"]
    # multi-GPU: gradients cross xGMI as bf16 (fp32 accumulation in the owner),
    # as the reference's fp16 O2 gradients do -- half the reduce-scatter bytes
    grad_wire = args.grad_reduce_dtype or ("bfloat16" if n > 1 else "float32")
    ov.append("Distributed.comm.reduce_dtype=%s" % grad_wire)
    graph = use_graph(args.hip_graph, n, args.warmup)
    ov.append("Engine.cuda_graph=%s" % bool(graph))
    # A/B experiments: extra config overrides, e.g. "Distributed.comm.early_grad_norm=False"
    ov += [o for o in os.environ.get("FLEETX_BENCH_OVERRIDES", "").split(";") if o]
    os.environ.setdefault("FLEETX_LOG_RANK0_ONLY", "1")
    cfg = cfgmod.get_config(cfg_file, overrides=ov, nranks=n)
    env.init_dist_env(cfg)
    env.set_seed(cfg.Global.seed)
    module = build_module(cfg)
    engine = EagerEngine(configs=cfg, module=module, mode="train")
    dev = engine.device
    hcg = engine.hcg
    V = cfg.Model.vocab_size
    S = args.seq
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + hcg.dp_rank)

    def batch():
        toks = torch.randint(0, V, (local_batch, S + 1), device=dev, generator=gen)
        pos = torch.arange(S, device=dev).unsqueeze(0).expand(local_batch, S)
        return [toks[:, :-1].contiguous(), pos, toks[:, 1:].contiguous(),
                torch.ones(local_batch, S, device=dev)]

    def step():
        return engine._fit_impl(batch())

    for _ in range(args.warmup):
        loss = step()
    sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)
    sync()
    if dist.is_initialized():
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    sync()
    if dist.is_initialized():
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    if dist.is_initialized():
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    lval = engine._reduce_log_loss(loss, 1)
    peak_mem = torch.cuda.max_memory_allocated() if torch.cuda.is_available() else None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, engine, module, lval, write=env.get_rank() == 0)
    tokens = global_batch * S * args.steps
    tps = tokens / elapsed
    fpt = flops_per_token(module.gpt_config, S)
    mfu = tps * fpt / (n * PEAK_BF16)
    par = "_".join(x for x in (
        "dp%d" % dp if dp > 1 else "", "sharding%d_stage%d" % (sharding, stage) if sharding > 1
        else "", "tp%d" % mp if mp > 1 else "", "pp%d" % pp if pp > 1 else "",
        "sp" if args.sequence_parallel and mp > 1 else "") if x) or "dp1"
    if env.get_rank() == 0:
        from fleetx_amd.ops import gemm as gemm_routes
        out = {
            "metric": "tokens/sec (whole node) GPT-3 6.7B hybrid-parallel at 1/2/4/8 MI355X"
            if args.model == "gpt3-6.7B" else "tokens/sec %s" % args.model,
            "value": round(tps, 1), "unit": "tokens/s", "n_gpus": n, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1000 * elapsed / args.steps, 2),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": round(tps / (REF_TOKENS_PER_GPU[args.model] * n), 3)
            if args.model in REF_TOKENS_PER_GPU else None,
            "dtype": "bf16" if engine._dtype == torch.bfloat16
            else str(engine._dtype).replace("torch.", ""),
            "data": "synthetic (random tokens), random-init weights",
            "config": {"model": args.model, "global_batch": global_batch, "seq_len": S,
                       "parallelism": par, "micro_batch": micro,
                       "layout": {"dp": dp, "tp": mp, "pp": pp, "sharding": sharding,
                                  "sharding_stage": stage, "micro_batch": micro,
                                  "accumulate_steps": local_batch // max(micro, 1),
                                  "schedule": "1F1B" if pp > 1 else "none",
                                  "source": "cli" if args.layout not in (None, "planner")
                                  else ("planner" if layout in (None, "planner")
                                        else "baseline-config3-family")},
                       "hip_graph": bool(getattr(engine, "_cuda_graph", False)),
                       "grad_reduce_dtype": grad_wire,
                       "dropout": drop, "recompute": recompute},
            "mfu": round(mfu, 4), "tokens_per_gpu": round(tps / n, 1),
            "final_loss": round(lval, 4),
            "peak_mem_gb": round(peak_mem / 2 ** 30, 1) if peak_mem is not None else None,
            # forward / data-gradient shapes routed to the MFMA kernel and
            # where each route came from (shipped plan or first-call race);
            # weight gradients follow the kind table (ops/gemm.py)
            "gemm_kernel_routes": gemm_routes.kernel_routes(),
        }
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
