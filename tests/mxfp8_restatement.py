"""The MXFP8 rule of include_staged/thunder_speech_amd/mxfp8.h restated in torch on the CPU, for tests/test_mxfp8_host.py, test_gpu_mxfp8_kernels.py
and test_gpu_mxfp8_encoder.py: the quantiser, the dequantiser, the hand-made blocks both quantiser tests share, and the fake-quantised
restatement of the encoder (oracle.w2v.forward's arithmetic with both operands of the four layer products passed through bf16 and the quantiser).

Quantiser, per block of 32 finite values v scaled in f32, amax = max|v|:  e = floor(log2 amax) - 8, + 1 if amax 2^-e > 448, clamped to [-127, 127];
scale byte e + 127; elements v 2^-e rounded to nearest-even to e4m3fn.  amax == 0: scale byte 0, element bytes 0.  The exponent and the comparison
come from the bits of amax.  torch's CPU cast to float8_e4m3fn is round-to-nearest-even and only returns NaN beyond 448, which the rule never
reaches."""
import torch

E4M3_MAX = 448.0


def mx_exponent(amax: torch.Tensor) -> torch.Tensor:
    """e (int32) of blocks with the given amax (f32, >= 0, finite)."""
    bits = amax.contiguous().view(torch.int32)
    e = (bits >> 23) - 135 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)       # mantissa above 1.75: amax 2^-e would exceed 448
    return e.clamp(-127, 127)


def mx_quantize(v: torch.Tensor):
    """v [..., k] (bf16 or f32, k % 32 == 0) -> (element bytes uint8 [..., k], scale bytes uint8 [..., k / 32])."""
    assert v.shape[-1] % 32 == 0
    blocks = v.to(torch.float32).reshape(*v.shape[:-1], v.shape[-1] // 32, 32)
    amax = blocks.abs().amax(-1)
    e = mx_exponent(amax)
    mult = ((127 - e) << 23).to(torch.int32).view(torch.float32)                  # 2^-e: a normal f32 for every e the rule gives
    q = (blocks * mult.unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where((amax == 0).unsqueeze(-1), torch.zeros_like(q), q)
    return q.reshape(v.shape), (e + 127).to(torch.uint8)


def mx_dequantize(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """float64 [..., k]: element value x 2^(scale byte - 127)."""
    vals = q.contiguous().view(torch.float8_e4m3fn).to(torch.float64).reshape(*q.shape[:-1], q.shape[-1] // 32, 32)
    return (vals * torch.pow(torch.tensor(2.0, dtype=torch.float64), scales.to(torch.float64) - 127.0).unsqueeze(-1)).reshape(q.shape)


def fake_quant(v: torch.Tensor) -> torch.Tensor:
    """v rounded to bf16 and passed through the quantiser along its last axis: the values an MX product multiplies, as f32."""
    q, s = mx_quantize(v.to(torch.bfloat16))
    return mx_dequantize(q, s).to(torch.float32)


def handmade_blocks() -> torch.Tensor:
    """f32 [n][32]: amax of 448, 449, 256 and 255.9 times powers of two (both signs), a zero block, a block of one tiny value, the lower clamp
    (amax 2^-125: e = -133 -> -127), the largest finite f32 (e = 120: no finite f32 reaches the upper clamp), elements that land on e4m3
    subnormals (a tie among them), and a block whose amax is negative."""
    rows = []
    g = torch.Generator().manual_seed(31)
    for base in (448.0, 449.0, 256.0, 255.9):
        for p in (0, -3, 5, -20):
            b = (torch.rand(32, generator=g) * 2 - 1) * base * 2.0 ** p * 0.999
            b[5] = base * 2.0 ** p
            b[9] = -0.37 * base * 2.0 ** p
            rows.append(b)
    rows.append(torch.zeros(32))
    z = torch.zeros(32); z[7] = -0.0; rows.append(z.clone())
    t = torch.zeros(32); t[17] = 1e-30; rows.append(t)
    lo = torch.zeros(32); lo[0] = 2.0 ** -125; lo[1] = -(2.0 ** -126); lo[2] = 2.0 ** -140; rows.append(lo)
    hi = torch.zeros(32); hi[3] = torch.finfo(torch.float32).max; hi[4] = -1e38; hi[5] = 1.0; rows.append(hi)
    sub = torch.zeros(32); sub[0] = 256.0                                          # e = 0: elements below 2^-6 are e4m3 subnormals (steps of 2^-9)
    sub[1:8] = torch.tensor([1.5, 2.5, 3.5, 0.5, 0.49, 7.6, -4.5]) * 2.0 ** -9     # ties at 1.5, 2.5, 3.5, 0.5, 4.5 steps: to even
    rows.append(sub)
    neg = -torch.rand(32, generator=g) * 3.0; neg[30] = -448.0 * 4; rows.append(neg)
    return torch.stack(rows).to(torch.float32)


def w2v_forward_fake_quant(cfg, sd, audio, lengths=None):
    """oracle.w2v.forward with both operands of the four products of every transformer layer (q / k / v, out_proj, the two feed-forward linears)
    replaced by fake_quant of themselves; everything else f32 as the oracle has it.  The oracle multiplies through torch.nn.functional.linear, which
    is patched for the layer products only while the oracle runs its encoder layers (the layer weights are recognised by identity)."""
    import torch.nn.functional as F
    from oracle import w2v as ow
    layer_w = set()
    for k, v in sd.items():
        if k.startswith("encoder.layers.") and k.endswith(".weight") and v.dim() == 2 and (
                ".attention." in k and "_proj." in k or ".feed_forward." in k):
            layer_w.add(k)
    sd2 = dict(sd)
    marked = {}
    for k in layer_w:
        sd2[k] = fake_quant(sd[k].float())
        marked[id(sd2[k])] = True
    real = F.linear

    def linear(x, w, b=None):
        if id(w) in marked:
            return real(fake_quant(x), w, b)
        return real(x, w, b)
    F.linear = linear
    try:
        return ow.forward(cfg, sd2, audio, lengths)
    finally:
        F.linear = real
