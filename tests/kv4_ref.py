"""The int4 KV cache format (include/gptq_mi355x.h "int4 KV cache") restated in PyTorch on the CPU -- the specification the kernels of
csrc/decode_attn_kv4.hip are tested against -- and a float64 attention over a dequantised cache: codes uint8 [..., heads * 64] (16 bytes per
group of 32 values), meta fp16 [..., heads, 4, 2] ({d, m} per group, the value is m + d c)."""
import torch

HD, GROUP = 128, 32
NIBBLE_OF = (0, 4, 1, 5, 2, 6, 3, 7)          # element i of a word sits in nibble NIBBLE_OF[i]
ELEMENT_AT = (0, 2, 4, 6, 1, 3, 5, 7)         # ... and nibble n holds element ELEMENT_AT[n]


def quantise(rows):
    """rows: fp16 [..., heads * 128] (CPU or GPU) -> (codes uint8 [..., heads * 64], meta fp16 [..., heads, 4, 2]) on the CPU"""
    r = rows.detach().cpu()
    assert r.dtype == torch.float16 and r.shape[-1] % HD == 0
    lead, heads = r.shape[:-1], r.shape[-1] // HD
    x = r.float().reshape(*lead, heads, 4, GROUP)
    m = x.amin(dim=-1, keepdim=True) + 0.0                      # (-0 -> +0: which zero a minimum returns is nobody's rule)
    d = (((x.amax(dim=-1, keepdim=True) + 0.0) - m) / 15.0).half()
    inv = 1.0 / d.float()
    c = torch.round((x - m) * inv).clamp(0, 15)                 # torch.round: to nearest even
    c = torch.where(d == 0, torch.zeros_like(c), c).to(torch.uint8)
    nib = c.reshape(*lead, heads, 4, 4, 8)[..., ELEMENT_AT]     # [..., word, nibble]
    codes = (nib[..., 0::2] | (nib[..., 1::2] << 4)).reshape(*lead, heads * 64)
    return codes, torch.cat([d, m.half()], dim=-1)


def dequantise(codes, meta):
    """(uint8 [..., heads * 64], fp16 [..., heads, 4, 2]) -> float64 [..., heads * 128]"""
    codes, meta = codes.detach().cpu(), meta.detach().cpu().double()
    lead, heads = codes.shape[:-1], meta.shape[-3]
    b = codes.reshape(*lead, heads, 4, 4, 4)
    nib = torch.stack([b & 15, b >> 4], dim=-1).reshape(*lead, heads, 4, 4, 8)
    c = nib[..., NIBBLE_OF].reshape(*lead, heads, 4, GROUP).double()
    return (meta[..., 1:2] + meta[..., 0:1] * c).reshape(*lead, heads * HD)


def attention(q_rot, k4, kmeta, v4, vmeta, length, scale):
    """one row of a decode batch: q_rot [heads * 128] (the rotated fp16 query), the row's cache slices, rows 0 .. length - 1 attended to
    -> float64 [heads * 128]"""
    heads = kmeta.shape[-3]
    K = dequantise(k4[:length], kmeta[:length]).reshape(length, heads, HD)
    V = dequantise(v4[:length], vmeta[:length]).reshape(length, heads, HD)
    q = q_rot.detach().cpu().double().reshape(heads, HD)
    p = torch.softmax(torch.einsum('hd,thd->ht', q, K) * float(scale), dim=-1)
    return torch.einsum('ht,thd->hd', p, V).reshape(heads * HD)
