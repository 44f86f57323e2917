"""Shared data for the exact int4 decode-GEMV layout tests (test_decode_w4_gpu.py)."""
import functools

import torch


@functools.lru_cache(maxsize=None)
def _int4_case(M, N, K, seed):
    """Integer x [M, K] in [-4, 4], int8 q [N, K] uniform over all 16 int4 codes
    [-8, 7], group scales ``s[g, n] = 2^-(5 + (3g + n) % 4)`` [K / 256, N] (a
    wrong group or column index changes the result), bias and residual in
    [-8, 8], and the float64 result ``sum_g (x_g q_g^T) s[g] + b``.

    Every term is a multiple of 2^-8 and ``sum |x| |q| s < 2^16``, so every
    partial sum in any order is a multiple of 2^-8 below 2^16: 24 bits, exact
    in fp32.  A kernel's output must equal the float64 result rounded once.
    Computed once per case and shared: callers leave the tensors unchanged."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (M, K), generator=g).double()
    q = torch.randint(-8, 8, (N, K), generator=g).to(torch.int8)
    b = torch.randint(-8, 9, (N,), generator=g).double()
    res = torch.randint(-8, 9, (M, N), generator=g).double()
    G = K // 256
    e = 5 + (3 * torch.arange(G)[:, None] + torch.arange(N)[None, :]) % 4
    scale = torch.pow(2.0, -e.double())                                   # [G, N]
    wd = q.double().view(N, G, 256) * scale.t()[:, :, None]
    bound = x.abs() @ wd.abs().view(N, K).t()
    assert float(bound.max()) < 2 ** 16
    ref = x @ wd.view(N, K).t() + b
    return x, q, scale.float(), b, res, ref
