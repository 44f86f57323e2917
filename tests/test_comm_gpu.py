"""One-shot IPC all-reduce (csrc/kernels/comm.hip, parallel/comm.py) on the GPU.

Two ranks share the one MI355X (IPC handles of the same device opened by the
peer process; the handle exchange runs over gloo).  Each rank's result is
compared against an fp32 torch reduction of every rank's input computed
locally from the shared seed: sum and max, fp32 / bf16 / fp16, sizes from one
element to the slot limit, many back-to-back calls (epoch parity), out of
place, and inside a captured HIP graph replayed with new data."""
import pytest
import torch

from tests import dist_utils

pytestmark = pytest.mark.gpu


def _inputs(world, n, dtype, it):
    g = torch.Generator().manual_seed(1000 * it + n)
    return [torch.randn(n, generator=g).to(dtype) for _ in range(world)]


def _oneshot(rank, world):
    import torch.distributed as dist
    from fleetx_amd.parallel.comm import IpcAllReduce
    torch.cuda.set_device(0)
    ar = IpcAllReduce(None, max_bytes=64 * 1024)
    worst = {}
    it = 0
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for n in (1, 2, 3, 255, 1024, 4097, 16384 if dtype == torch.float32 else 32768):
            for op in (dist.ReduceOp.SUM, dist.ReduceOp.MAX):
                it += 1
                xs = _inputs(world, n, dtype, it)
                x = xs[rank].cuda()
                y = ar.all_reduce(x.clone(), op)
                ref = torch.stack([t.float() for t in xs])
                ref = ref.sum(0) if op == dist.ReduceOp.SUM else ref.max(0).values
                err = (y.float().cpu() - ref).abs().max().item()
                key = (str(dtype), int(op == dist.ReduceOp.MAX))
                worst[key] = max(worst.get(key, 0.0), err)
    # out of place, 200 back-to-back calls without host syncs
    acc = []
    for i in range(200):
        x = torch.full((777,), float(rank + i), device="cuda")
        out = torch.empty_like(x)
        ar.all_reduce(x, out=out)
        acc.append(out[0:1])
    seq = torch.cat(acc).cpu()
    expect = torch.tensor([float(sum(r + i for r in range(world))) for i in range(200)])
    # graph capture: the epochs live on the device, so replays keep working
    static = torch.zeros(4096, device="cuda")
    ar.all_reduce(static.clone())
    torch.cuda.synchronize()
    dist.barrier()
    gr = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            res = ar.all_reduce(static.clone())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    dist.barrier()
    graph_ok = []
    for i in range(5):
        static.fill_(float(10 * i + rank))
        gr.replay()
        torch.cuda.synchronize()
        graph_ok.append(float(res[123].item()))
    ar.check()
    torch.cuda.synchronize()
    dist.barrier()
    ar.close()
    return worst, bool(torch.equal(seq, expect)), graph_ok


def test_oneshot_allreduce_two_ranks_one_gpu():
    res = dist_utils.run(_oneshot, 2, timeout=300)
    for worst, seq_ok, graph in res:
        assert seq_ok
        assert graph == [float(sum(10 * i + r for r in range(2))) for i in range(5)]
        for (dt, is_max), e in worst.items():
            if is_max:
                assert e == 0.0, (dt, e)
            else:
                tol = 1e-6 if "float32" in dt else (0.07 if "bfloat16" in dt else 0.01)
                assert e <= tol, (dt, e)
    # all ranks see bitwise-identical results
    assert res[0][0] == res[1][0]


def _late_peer(rank, world):
    """Rank 1 calls 2 s after rank 0 with a 0.5 s timeout: rank 0's call must
    come back as NaN with the error flag raised (never a normal-looking
    result), rank 1's call completes correctly, and once rank 0 has seen the
    error the next call of both ranks is correct again (the protocol survives
    a timeout)."""
    import time
    import torch.distributed as dist
    from fleetx_amd.parallel.comm import IpcAllReduce, OneShotTimeout
    torch.cuda.set_device(0)
    ar = IpcAllReduce(None, max_bytes=16 * 1024, timeout_s=0.5)
    x = torch.full((1000,), float(rank + 1), device="cuda")
    dist.barrier()
    if rank == 1:
        time.sleep(2.0)
    y = ar.all_reduce(x.clone())
    torch.cuda.synchronize()
    first = y.cpu()
    raised = False
    try:
        ar.check()
    except OneShotTimeout as e:
        raised = "timed out" in str(e)
        # acknowledge the error: while the flag is set a call does not wait for
        # its peers at all, so the next result would depend on which rank's
        # kernel starts first after the barrier
        ar.err.zero_()
    dist.barrier()
    z = ar.all_reduce(torch.full((1000,), float(10 * (rank + 1)), device="cuda"))
    torch.cuda.synchronize()
    second = z.cpu()
    dist.barrier()
    ar.close()
    return bool(torch.isnan(first).all()), bool((first == 3.0).all()), raised, \
        bool((second == 30.0).all())


def test_oneshot_timeout_poisons_and_raises():
    res = dist_utils.run(_late_peer, 2, timeout=300)
    nan0, ok0, raised0, next0 = res[0]
    nan1, ok1, raised1, next1 = res[1]
    assert nan0 and raised0, res[0]          # the waiting rank: NaN + flag
    assert ok1 and not raised1, res[1]       # the late rank found rank 0's data
    assert next0 and next1                   # the following call is correct on both
