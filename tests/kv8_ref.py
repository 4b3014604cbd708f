"""The fp8 KV cache format (include/gptq_mi355x.h "fp8 KV cache") restated in PyTorch on the CPU -- the specification the kernels of
csrc/decode_attn_kv8.hip are tested against -- and a float64 attention over a dequantised cache.

    k8 / v8      uint8 [..., heads * 128]   OCP e4m3fn bytes
    kexp / vexp  int8  [..., heads]         one exponent e per (token, head): the stored head row means q_i * 2^e

A head row r[0 .. 128) of fp16 values: amax = max |r_i|; e = 0 when amax == 0, else the smallest integer with amax * 2^-e <= 448
(amax = m * 2^x, m in [0.5, 1): e = x - 9 when m <= 0.875, else x - 8); q_i = RNE_e4m3(r_i * 2^-e) = torch.ldexp(r.float(), -e).to(float8_e4m3fn).
"""
import torch

HD = 128
E4M3_MAX = 448.0


def exponents(rows):
    """rows: fp16 [..., heads, 128] -> int32 [..., heads]"""
    amax = rows.detach().cpu().float().abs().amax(dim=-1)
    m, x = torch.frexp(amax)                                   # amax = m * 2^x, m in [0.5, 1)
    e = x.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def quantise(rows):
    """rows: fp16 [..., heads * 128] (CPU or GPU) -> (bytes uint8 [..., heads * 128], exponents int8 [..., heads]) on the CPU"""
    r = rows.detach().cpu()
    assert r.dtype == torch.float16 and r.shape[-1] % HD == 0
    heads = r.shape[-1] // HD
    r = r.reshape(*r.shape[:-1], heads, HD)
    e = exponents(r)
    q = torch.ldexp(r.float(), (-e).unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).reshape(*r.shape[:-2], heads * HD), e.to(torch.int8)


def dequantise(q8, e8):
    """(uint8 [..., heads * 128], int8 [..., heads]) -> float64 [..., heads * 128]"""
    q8, e8 = q8.detach().cpu(), e8.detach().cpu()
    heads = e8.shape[-1]
    f = q8.view(torch.float8_e4m3fn).float().double().reshape(*e8.shape, HD)
    return torch.ldexp(f, e8.to(torch.int32).unsqueeze(-1)).reshape(*q8.shape[:-1], heads * HD)


def attention(q_rot, k8, kexp, v8, vexp, length, scale):
    """one row of a decode batch: q_rot [heads * 128] (the rotated fp16 query), the row's cache slices (k8 / v8 [t_max, heads * 128], kexp / vexp
    [t_max, heads]), rows 0 .. length - 1 attended to -> float64 [heads * 128]"""
    heads = kexp.shape[-1]
    K = dequantise(k8[:length], kexp[:length]).reshape(length, heads, HD)
    V = dequantise(v8[:length], vexp[:length]).reshape(length, heads, HD)
    q = q_rot.detach().cpu().double().reshape(heads, HD)
    s = torch.einsum('hd,thd->ht', q, K) * float(scale)
    p = torch.softmax(s, dim=-1)
    return torch.einsum('ht,thd->hd', p, V).reshape(heads * HD)


def random_rows(gen, shape_rows, heads, zero_rows=0.03, spike_rows=0.03):
    """fp16 [*shape_rows, heads * 128] test rows off unit scale: every head row N(0, 1) x 2^U(-6, 6), a few head rows all zero, a few with one
    element 1 000 x the rest (CPU generator `gen`)"""
    n = 1
    for d in shape_rows:
        n *= d
    x = torch.randn((n * heads, HD), generator=gen)
    x *= torch.exp2(torch.rand((n * heads, 1), generator=gen) * 12 - 6)
    pick = torch.rand(n * heads, generator=gen)
    x[pick < zero_rows] = 0
    spike = (pick >= zero_rows) & (pick < zero_rows + spike_rows)
    col = torch.randint(0, HD, (n * heads,), generator=gen)
    idx = spike.nonzero().reshape(-1)
    x[idx, col[idx]] *= 1000.0
    return x.clamp_(-60000, 60000).half().reshape(*shape_rows, heads * HD)
