"""ts_qn_head_fwd (csrc/qn_head.hip, include_open/thunder_speech_amd/qn_head.h): QuartzNet's last 1x1 block and the conv1d CTC decoder as one launch,
through the C ABI against a float64 restatement per element, and through BaseCTCModule against the two launches it replaces.

The restatement reads the operands the device holds: x rounded to bf16 with zeros from the clip's length on (the tail-zero invariant), the folded
weights W17 and the decoder's Wd rounded to bf16, the f32 shift b17 and bias bd.  In float64:
    pre = b17 + W17 x,   h = bf16(relu(pre)) (0 from len[b] on when lengths are given),   logits = bd + Wd h
Bound, per element, derived as tests/test_gpu_tcs_kernels.py derives pw_logits' (u16 = 2^-8, u32 = 2^-24; products of two bf16 values are exact in f32):
  1. pre accumulates c_in products on top of the shift in f32 (+ 1: the restatement passes its own pre through f32 on the way to bf16):
                                                                               e_pre = (c_in + 2) u32 P1,   P1 = |b17| + |W17| |x|
  2. h.  Device and restatement each round THEIR pre to bf16; |rn(a) - rn(b)| <= |a - b| + u16 (|a| + |b|):
                                                                               E_h = e_pre + u16 (2 |relu(pre)| + e_pre);   0 on masked frames
  3. logits: an f32 sum of `hidden` exact products, the bias and the seven joins of the eight waves' partial sums:
                                                                               E = |Wd| E_h + (hidden + 8) u32 (|bd| + |Wd| (|h| + E_h))
The module-level tests compare the fused launch with the two launches it replaces.  Both form h with the same instruction on the same operands in the
same order, so h is the same bf16 tensor in both and only step 3 separates them: each is within
                                                                               E_sum = (hidden + 8) u32 (|bd| + |Wd| |h|)
of the exact sum over that h, and they are within 2 E_sum of each other.  (Against float64 E_sum alone would not do: where the device's f32 pre and
the restatement's pre fall on different sides of a bf16 rounding boundary h differs by an ulp, which is what E_h accounts for; every kernel case
prints its ratio against E_sum as well, without asserting it.)
Nothing is fitted to measured ratios; every check prints `RATIO|what|largest error / bound` before it asserts.  The logits live inside a NaN-filled
buffer: frames from t_out to the pitch and the guard rows around the tensor must come back untouched."""
import ctypes as C

import pytest
import torch

U16, U32 = 2.0 ** -8, 2.0 ** -24
BF = torch.bfloat16
GUARD_ROWS = 4
_KEPT = []


def _lib():
    from thunder_speech_amd import _lib as L
    return L


def _operands(seed, batch, c_in, hidden, v, t, lengths):
    """CPU operands: what the device will hold (bf16-rounded where it holds bf16), as float32 / float64 tensors."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, c_in, t, generator=g).to(BF)
    lens = [t] * batch if lengths is None else list(lengths)
    for b, n in enumerate(lens):
        x[b, :, n:] = 0                                                    # the tail-zero invariant
    w17 = (torch.randn(hidden, c_in, generator=g) / c_in ** 0.5)
    b17 = 0.5 * torch.randn(hidden, generator=g)
    wd = 4.0 * torch.randn(v, hidden, generator=g) / hidden ** 0.5
    bd = torch.randn(v, generator=g)
    return dict(x=x, w17=w17, b17=b17, wd=wd, bd=bd, lens=lens, masked=lengths is not None, shape=(batch, c_in, hidden, v, t))


def _reference(op):
    """float64: (logits, bound E, E_sum)."""
    batch, c_in, hidden, v, t = op["shape"]
    x = op["x"].double()
    w17, wd = op["w17"].to(BF).double(), op["wd"].to(BF).double()
    b17, bd = op["b17"].double(), op["bd"].double()
    pre = torch.einsum("ck,bkt->bct", w17, x) + b17[None, :, None]
    p1 = torch.einsum("ck,bkt->bct", w17.abs(), x.abs()) + b17.abs()[None, :, None]
    e_pre = (c_in + 2) * U32 * p1
    r = pre.clamp_min(0)
    h = r.to(torch.float32).to(BF).double()                                # (pre in float64 -> f32 -> bf16: the f32 step changes nothing a bf16 sees
    e_h = e_pre + U16 * (2 * r + e_pre)                                    #  beyond e_pre's own margin)
    if op["masked"]:
        keep = (torch.arange(t)[None, :] < torch.tensor(op["lens"])[:, None])[:, None, :].double()
        h, e_h = h * keep, e_h * keep
    ref = torch.einsum("vc,bct->bvt", wd, h) + bd[None, :, None]
    bound = torch.einsum("vc,bct->bvt", wd.abs(), e_h) + (hidden + 8) * U32 * (bd.abs()[None, :, None] + torch.einsum("vc,bct->bvt", wd.abs(), h.abs() + e_h))
    bound_sum = (hidden + 8) * U32 * (bd.abs()[None, :, None] + torch.einsum("vc,bct->bvt", wd.abs(), h.abs()))
    return ref, bound, bound_sum


def _device_operands(op, dev):
    from thunder_speech_amd import plan
    L = _lib()
    batch, c_in, hidden, v, t = op["shape"]
    pitch = L.time_pitch(t)
    xd = torch.zeros(batch, c_in, pitch, dtype=BF, device=dev)
    xd[:, :, :t] = op["x"].to(dev)
    d = dict(x=xd, w17=plan.pack_pw_frags16(op["w17"]).to(dev), b17=op["b17"].float().to(dev), wd=plan.pack_head_wd(op["wd"]).to(dev),
             bd=op["bd"].float().to(dev), len=torch.tensor(op["lens"], dtype=torch.int32, device=dev) if op["masked"] else None, pitch=pitch)
    _KEPT.append(d)
    return d


def _launch(op, d, out_pitch=None):
    """One call; returns (status, whole NaN-filled buffer, view of the logits inside it)."""
    L = _lib()
    batch, c_in, hidden, v, t = op["shape"]
    pitch_out = out_pitch or L.time_pitch(t)
    buf = torch.full((batch * v + 2 * GUARD_ROWS, pitch_out), float("nan"), dtype=torch.float32, device=d["x"].device)
    y = buf[GUARD_ROWS: GUARD_ROWS + batch * v].view(batch, v, pitch_out)
    st = L.lib().ts_qn_head_fwd(d["x"].data_ptr(), None if d["len"] is None else d["len"].data_ptr(), d["w17"].data_ptr(), d["b17"].data_ptr(),
                                d["wd"].data_ptr(), d["bd"].data_ptr(), y.data_ptr(), batch, c_in, hidden, v, t, d["pitch"], pitch_out, 1, 1, 0,
                                torch.cuda.current_stream().cuda_stream)
    _KEPT.append(buf)
    return st, buf, y


def _check(what, op, buf, y, ref, bound, bound_sum):
    batch, c_in, hidden, v, t = op["shape"]
    got = y[:, :, :t].double().cpu()
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"RATIO|{what}|{ratio:.3e}")
    print(f"RATIO|{what} (against E_sum, not asserted)|{float((err / bound_sum.clamp_min(1e-300)).max()):.3e}")
    assert bool(torch.isfinite(got).all()), what
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), f"{what}: error {float(err.flatten()[worst]):.3e} > bound {float(bound.flatten()[worst]):.3e} (largest error / bound {ratio:.3e})"
    assert bool(torch.isnan(y[:, :, t:]).all()), f"{what}: frames beyond t_out were written"
    assert bool(torch.isnan(buf[:GUARD_ROWS]).all()) and bool(torch.isnan(buf[-GUARD_ROWS:]).all()), f"{what}: guard rows were written"
    if op["masked"]:                                                       # masked frames: h is exactly 0, the logits are exactly the bias
        for b, n in enumerate(op["lens"]):
            assert torch.equal(y[b, :, n:t].cpu(), op["bd"].float()[:, None].expand(v, t - n)), f"{what}: masked frames of clip {b}"


CASES = {
    # three full tiles plus a 45-frame one; a clip that ends inside the second tile; an empty clip
    "3x512-1024-29xT333-lengths": dict(seed=1, batch=3, c_in=512, hidden=1024, v=29, t=333, lengths=(333, 97, 0)),
    "one-full-tile": dict(seed=2, batch=2, c_in=512, hidden=1024, v=29, t=96, lengths=None),
    "one-frame": dict(seed=3, batch=2, c_in=512, hidden=1024, v=29, t=1, lengths=None),
    "v32": dict(seed=4, batch=2, c_in=512, hidden=1024, v=32, t=100, lengths=(100, 51)),
    "hidden512-one-pass": dict(seed=5, batch=2, c_in=512, hidden=512, v=29, t=100, lengths=None),
    "cin256": dict(seed=6, batch=2, c_in=256, hidden=1024, v=29, t=100, lengths=(33, 100)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_head_matches_float64_restatement(name):
    L = _lib()
    op = _operands(**CASES[name])
    ref, bound, bound_sum = _reference(op)
    d = _device_operands(op, "cuda")
    n0 = L.lib().ts_qn_head_launches()
    st, buf, y = _launch(op, d)
    assert st == 0, st
    assert L.lib().ts_qn_head_launches() == n0 + 1
    torch.cuda.synchronize()
    _check(name, op, buf, y, ref, bound, bound_sum)
    assert float(ref.abs().max()) > 1.0


@pytest.mark.gpu
def test_two_calls_give_the_same_bits():
    op = _operands(seed=7, batch=3, c_in=512, hidden=1024, v=29, t=333, lengths=(333, 200, 5))
    d = _device_operands(op, "cuda")
    st1, _, y1 = _launch(op, d)
    st2, _, y2 = _launch(op, d)
    torch.cuda.synchronize()
    assert st1 == 0 and st2 == 0
    assert torch.equal(y1[:, :, :333].cpu().view(torch.int32), y2[:, :, :333].cpu().view(torch.int32))


@pytest.mark.gpu
def test_back_to_back_launches_on_different_inputs_each_match_their_own_restatement():
    """Two launches queued without a synchronisation in between: nothing of the first (its LDS image, its weight ring) may reach the second."""
    ops = [_operands(seed=8, batch=2, c_in=512, hidden=1024, v=29, t=200, lengths=(200, 120)),
           _operands(seed=9, batch=2, c_in=512, hidden=1024, v=29, t=200, lengths=None)]
    refs = [_reference(op) for op in ops]
    ds = [_device_operands(op, "cuda") for op in ops]
    torch.cuda.synchronize()
    outs = [_launch(op, d) for op, d in zip(ops, ds)]
    torch.cuda.synchronize()
    for i, (op, (st, buf, y), (ref, bound, bound_sum)) in enumerate(zip(ops, outs, refs)):
        assert st == 0
        _check(f"back-to-back-{i}", op, buf, y, ref, bound, bound_sum)


# ---------------------------------------------------------------------------------------------------------------------
# module level: QuartzNet5x5 with the switch on against the switch off
# ---------------------------------------------------------------------------------------------------------------------
_MODULE = {}


def _module():
    if "m" not in _MODULE:
        from oracle import tcs as otcs
        from thunder_speech_amd.quartznet.compatibility import build_synthetic_quartznet
        arch = otcs.quartznet_arch(repeat_blocks=1)
        sd = otcs.synth_encoder_state(arch, seed=0, calibrate=True)
        dsd = otcs.synth_decoder_state(1024, 29, seed=1, gain=4.0)
        _MODULE["m"] = build_synthetic_quartznet(repeat_blocks=1, encoder_state=sd, decoder_state=dsd).to("cuda").eval()
    m = _MODULE["m"]
    m.eval()
    m.fused_head, m.graph_inference = True, False
    return m


def _unpack_frags16(fr):
    """[Cout / 16][Cin / 32][64][8] -> [Cout][Cin]: the inverse of plan.pack_pw_frags16."""
    n16, k32 = fr.shape[:2]
    return fr.view(n16, k32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(n16 * 16, k32 * 32)


def _head_bound(m, wav, lengths):
    """E_sum of the restatement above for this module and input, from the tensor the last block reads."""
    from thunder_speech_amd import tensors as _t
    enc = m.encoder
    with torch.no_grad(), _t.lengths_scope():
        feats, fl = m.audio_transform(wav, lengths)
        x = _t.pack(feats, fl, slot=("test-head", 0))
        blocks = list(enc.children())
        for i, blk in enumerate(blocks[:-1]):
            x, fl, _ = blk._run_fused(x, fl, internal=True, slot=("test-head", i % 2))
        torch.cuda.synchronize()
        x = x.float().cpu()
    last = blocks[-1]
    layer = last._cache.get(last._params(), last._compile)[0]
    b, c_in, t = x.shape
    op = dict(x=x.to(BF), w17=_unpack_frags16(layer.pw16.cpu()).float(), b17=layer.bias.cpu()[: layer.c_out],
              wd=m.decoder.weight.detach().cpu().reshape(m.decoder.out_channels, -1), bd=m.decoder.bias.detach().cpu(), lens=[t] * b, masked=False,
              shape=(b, c_in, layer.c_out, m.decoder.out_channels, t))
    return _reference(op)[2]


@pytest.mark.gpu
@pytest.mark.parametrize("batch,seconds,seed", [(2, 2, 11), (4, 10, 75)])
def test_module_fused_head_against_the_two_launches(batch, seconds, seed):
    from thunder_speech_amd.module import greedy_decode
    L = _lib()
    m = _module()
    g = torch.Generator().manual_seed(seed)
    wav = (0.1 * torch.randn(batch, 16000 * seconds, generator=g)).cuda()
    lengths = torch.full((batch,), 16000 * seconds, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        n0 = L.lib().ts_qn_head_launches()
        fused, len_f = m(wav, lengths)
        assert L.lib().ts_qn_head_launches() == n0 + 1, "the fused head did not serve the forward"
        m.fused_head = False
        plain, len_p = m(wav, lengths)
        assert L.lib().ts_qn_head_launches() == n0 + 1, "the switch did not switch the fused head off"
        ids_f, col_f, cnt_f = greedy_decode(fused)
        ids_p, col_p, cnt_p = greedy_decode(plain)
    torch.cuda.synchronize()
    assert torch.equal(len_f, len_p) and fused.shape == plain.shape and fused.dtype == plain.dtype == torch.float32
    bound = _head_bound(m, wav, lengths)
    diff = (fused.double().cpu() - plain.double().cpu()).abs()
    ratio = float((diff / (2 * bound).clamp_min(1e-300)).max())
    print(f"RATIO|module {batch}x{seconds}s fused vs two launches|{ratio:.3e}")
    assert bool((diff <= 2 * bound).all()), ratio
    # frames decided by less than twice the bound (of the two classes in question) may go either way; the seeds keep them under the cap -- chosen
    # on the two-launch output alone: with these random weights noise clips of 4 x 10 s have 2 to 14 such frames in 2004, seed 75 has 2
    top2 = plain.double().cpu().topk(2, dim=1)
    close = (top2.values[:, 0] - top2.values[:, 1]) <= 2 * bound.gather(1, top2.indices).max(dim=1).values
    share = float(close.double().mean())
    print(f"RATIO|module {batch}x{seconds}s share of frames with a top-2 margin below twice the bound|{share:.3e}")
    assert share <= 1e-3, share
    same = (ids_f == ids_p).cpu()
    assert bool((same | close).all()), "ids differ on a frame whose margin exceeds twice the bound"
    for b in range(batch):
        if bool(same[b].all()):
            assert int(cnt_f[b]) == int(cnt_p[b]) and torch.equal(col_f[b, : int(cnt_f[b])], col_p[b, : int(cnt_p[b])])


@pytest.mark.gpu
def test_graph_replay_equals_eager_bit_for_bit():
    L = _lib()
    m = _module()
    g = torch.Generator().manual_seed(13)
    wav = (0.1 * torch.randn(2, 32000, generator=g)).cuda()
    lengths = torch.full((2,), 32000, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        eager, _ = m._forward_eager(wav, lengths)
        eager = eager.clone()
        m.graph_inference = True
        stamp_on = m._weights_stamp()
        outs = [m(wav, lengths)[0] for _ in range(3)]
        graphs = m.__dict__["_infer_graphs"]
        assert graphs[1].count() + graphs[2].count() >= 1, "no inference graph was captured"
        n0 = L.lib().ts_qn_head_launches()
        outs.append(m(wav, lengths)[0])                                    # a replay: no call of the entry point
        assert L.lib().ts_qn_head_launches() == n0
        m.fused_head = False
        assert m._weights_stamp() != stamp_on, "the switch is not part of the inference graphs' stamp"
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o.view(torch.int32), eager.view(torch.int32))
    m.graph_inference = False


@pytest.mark.gpu
def test_fallback_under_hook_train_and_requires_grad():
    L = _lib()
    m = _module()
    g = torch.Generator().manual_seed(14)
    wav = (0.1 * torch.randn(2, 16000, generator=g)).cuda()
    lengths = torch.full((2,), 16000, dtype=torch.int32, device="cuda")
    count = L.lib().ts_qn_head_launches
    with torch.no_grad():
        n0 = count()
        ref, _ = m(wav, lengths)
        assert count() == n0 + 1
        seen = []
        hook = m.decoder.register_forward_hook(lambda mod, inp, out: seen.append(tuple(inp[0].shape)))
        try:
            hooked, _ = m(wav, lengths)
        finally:
            hook.remove()
        assert count() == n0 + 1 and seen and seen[0][1] == 1024, "a decoder hook must see the 1024-channel tensor"
        enc, _ = m.encoder(*m.audio_transform(wav, lengths))
        assert enc.shape[1] == 1024 and count() == n0 + 1                  # the encoder on its own still returns its last block's output
        m.train()
        try:
            assert not m._fused_head_ok(wav)
            m(wav, lengths)
        finally:
            m.eval()
        assert count() == n0 + 1
    wav_g = wav.clone().requires_grad_(True)
    m(wav_g, lengths)
    assert count() == n0 + 1
    with torch.no_grad():
        m(wav, lengths)
    assert count() == n0 + 2
    torch.cuda.synchronize()
    assert hooked.shape == ref.shape
