"""Pins the CPU restatements of tests/test_gpu_data_text_optim_kernels.py and tests/test_gpu_data_text_optim_bounded_kernels.py against the committed
fixtures and oracle/, without a GPU: collate, text encode and the SpecAugment tables against tests/golden/r2_misc.npz (generated from the reference),
the edit distance against oracle.metrics, audio preparation against oracle.dataprep, the mask draws against oracle.augment.draw_table, AdamW against
torch.optim.AdamW in float64 -- and measures, from the restatement alone, how many of the drawn spans probe the truncation boundary."""
import math

import numpy as np
import torch

import test_gpu_data_text_optim_bounded_kernels as B
import test_gpu_data_text_optim_kernels as K
from oracle import augment as oaug, dataprep as odp, metrics as omet


def test_restatements_match_the_reference_fixtures_and_the_oracle(golden):
    g = golden("r2_misc.npz")
    # collate: the fixture's clips in the order the reference sorted them
    clips = [torch.from_numpy(g[f"collate_clip{i}"]).reshape(-1) for i in g["collate_order"].tolist()]
    assert torch.equal(K.collate_reference(clips, g["collate_audio"].shape[1]), torch.from_numpy(g["collate_audio"]))
    assert K.collate_lengths(7, 5) == [7, 1, 1, 1, 3] and K.collate_lengths(1027, 5) == [1027, 1, 512, 513, 515] and K.collate_lengths(1, 5) == [1] * 5
    # text encode: QuartzNet labels, ids in label order; start / end / unknown appended behind them, pad = blank behind those
    labels = [" "] + [chr(ord("a") + i) for i in range(26)] + ["'"]
    vocab = {ord(c): i for i, c in enumerate(labels)}
    rows = [[ord(c) for c in str(s)] for s in g["enc_texts"]]
    blank, unk, bos, eos = len(labels), len(labels) + 1, len(labels) + 2, len(labels) + 3
    out, lens = K.encode_reference(rows, vocab, -1, -1, -1, blank, g["enc1"].shape[1])
    assert np.array_equal(out, g["enc1"]) and np.array_equal(lens, g["len1"])
    rows = [[ord(c) for c in str(s)] for s in g["enc_texts_unk"]]
    out, lens = K.encode_reference(rows, vocab, unk, bos, eos, blank, g["enc2"].shape[1])
    assert np.array_equal(out, g["enc2"]) and np.array_equal(lens, g["len2"])
    # SpecAugment / SpecCutout: the reference's host draws (torch.rand(1) twice per span) through the span arithmetic, and the rectangles applied
    x = torch.from_numpy(g["spec_x"])
    for name in ("specaug0", "specaug1", "specaug2"):
        n_time, tw, n_freq, fw = [int(v) for v in g[f"{name}_cfg"]]
        torch.manual_seed(int(g[f"{name}_seed"]))
        u = np.array([float(torch.rand(1)) for _ in range(2 * (n_time + n_freq))], dtype=np.float32).reshape(-1, 2)
        t0, t1, _ = K.spans_reference(u[:n_time, 0], u[:n_time, 1], tw, x.shape[2])
        f0, f1, _ = K.spans_reference(u[n_time:, 0], u[n_time:, 1], fw, x.shape[1])
        table = np.concatenate([np.stack([np.zeros_like(t0), np.full_like(t0, x.shape[1]), t0, t1], 1), np.stack([f0, f1, np.zeros_like(f0), np.full_like(f0, x.shape[2])], 1)])
        assert np.array_equal(table.astype(np.int32), g[f"{name}_table"]), name
    assert torch.equal(K.mask_reference(x, g["specaug0_table"].tolist()), torch.from_numpy(g["specaug0_y"]))
    assert torch.equal(K.mask_reference(x, g["cutout0_table"].tolist()), torch.from_numpy(g["cutout0_y"]))
    for name, table in K.MASK_TABLES.items():
        assert torch.equal(K.mask_reference(x, table), oaug.apply_table(x, np.array([[f0, f1 if f1 >= 0 else 0, t0, t1 if t1 >= 0 else 0] for f0, f1, t0, t1 in table])))
    # the Philox draws: the vectorised restatement against the oracle's row-by-row one
    for seed in K.DRAW_SEEDS[:3]:
        for (n_mels, n_frames) in K.DRAW_GEOMETRIES:
            for tw, fw, cfw in K.draw_widths(n_mels, n_frames):
                want = oaug.draw_table(oaug.philox_rand2(seed), n_mels, n_frames, n_time=7, time_width=tw, n_freq=6, freq_width=fw, n_cutout=5, cut_time_width=999,
                                       cut_freq_width=cfw)
                got, _ = K.draw_reference(seed, n_mels, n_frames, 7, tw, 6, fw, 5, cfw)
                assert np.array_equal(got, want), (seed, n_mels, n_frames, tw, fw, cfw)
    # edit distance
    for a, b in K.edit_pairs_small()[:9] + K.edit_pairs_small()[11:18]:
        assert K.edit_distance_reference(a, b) == omet.edit_distance(a, b), (len(a), len(b))
    # bf16 rounding of the adversarial values: what torch does on the CPU is round to nearest even on the bit pattern
    adv = K.adversarial_f32()
    w = adv.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    rne = ((w + 0x7FFF + ((w >> 16) & 1)) >> 16) & 0xFFFF
    bits, nan = K.bf16_round_bits(adv)
    assert int(nan.sum()) == 6 and torch.equal((bits.to(torch.int64) & 0xFFFF)[~nan], rne[~nan])
    # lengths: torch's floor division against Python's on the integers
    x = K.lengths_inputs(1)
    for add, div, plus in K.TRIPLES + K.INT_ONLY_TRIPLES:
        assert K.lengths_reference(x, add, div, plus, 1).tolist() == [(int(v) + add) // div + plus for v in x.tolist()]
        assert K.lengths_reference(K.lengths_inputs(0), add, abs(div), plus, 1).tolist() == [math.floor((float(v) + add) / abs(div)) + plus for v in K.lengths_inputs(0).tolist()]
    assert K.TRIPLES[1:5] == [(-1, 2, 1), (-1, 1, 1), (-1, 3, 1), (-1, 1, 1)]
    # im2col: against unfold on a full-length clip
    xs = torch.arange(1, 2 * 5 * 20 + 1, dtype=torch.int16).view(2, 5, 20).numpy()
    for k, s, d, p in [(3, 1, 1, 1), (5, 2, 1, 2), (3, 1, 2, 2), (7, 2, 3, 20)]:
        t_out = K.conv_t_out(17, k, s, d, p)
        got = K.im2col_reference(xs, None, 17, k, s, d, p, t_out, t_out)
        want = torch.nn.functional.unfold(torch.from_numpy(xs[:, :, :17]).float()[:, :, None, :], (1, k), dilation=(1, d), padding=(0, p), stride=(1, s))
        assert np.array_equal(got.reshape(2, k, 5, t_out), want.view(2, 5, k, t_out).permute(0, 2, 1, 3).numpy().astype(np.int16))
    # audio preparation
    from thunder_speech_amd.data.dataset import _sinc_kernel
    for channels, rate, t in B.AUDIO_CASES:
        audio = B.audio_clip(channels, t, rate + t)
        kern, width, orig, new = (None, 0, 1, 1) if rate == 16000 else _sinc_kernel(rate, 16000)
        if kern is not None:
            ok, ow, oo, on = odp.sinc_resample_kernel(rate, 16000)
            assert (ow, oo, on) == (width, orig, new) and float((ok[:, 0] - kern).abs().max()) <= 2.0 ** -24
        ref, bound = B.audio_prep_restate(audio, kern, orig, new, width)
        want = odp.preprocess_audio(audio, rate, True, 16000)
        assert want.shape == (1, ref.numel())
        assert float((ref - want[0].double()).abs().max()) <= 2e-5 and bool(((ref - want[0].double()).abs() <= bound).all())      # f32 in any order obeys the bound too
    # AdamW: the float64 restatement at double hyper-parameters is torch.optim.AdamW
    for step in (1, 2, 100):
        ops = B.adamw_operands(1025, step)
        want = B.torch_adamw_double(*ops, 1e-3, (0.9, 0.999), 1e-8, 1e-2, step)
        got = B.adamw_restate(*[o.double() for o in ops], 1e-3, 0.9, 0.999, 1e-8, 1e-2, step, bound=False)
        assert float((got["p"] - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert abs(B.beta2_first_order(0.999, 1) - 1.29e-5) < 1e-7
    # decoder gradient
    gl, xb = torch.randn(2, 3, 9), torch.randn(2, 4, 9).to(torch.bfloat16)
    w, ew, b, eb = B.decoder_bwd_restate(gl, xb)
    conv_w = torch.zeros(3, 4, 1, dtype=torch.float64, requires_grad=True)
    conv_b = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.conv1d(xb.double(), conv_w, conv_b) * gl.double()).sum().backward()
    assert torch.allclose(w, conv_w.grad[:, :, 0], rtol=1e-12, atol=1e-12) and torch.allclose(b, conv_b.grad, rtol=1e-12, atol=1e-12) and bool((ew > 0).all())


def test_the_draw_sweep_probes_the_truncation_boundary():
    """From the restatement's draws alone: the share of spans whose min_value lies within 1e-3 of an integer, per launch of the GPU test.  Uniform draws
    over a range of many units give 2e-3; 1 % is out of reach at these geometries (see the GPU file's docstring), so each launch must reach 1e-3 and
    the whole sweep several hundred spans."""
    shares, total = [], 0
    for n_mels, n_frames in K.DRAW_GEOMETRIES:
        for tw, fw, cfw in K.draw_widths(n_mels, n_frames):
            for seed in K.DRAW_SEEDS:
                _, mv = K.draw_reference(seed, n_mels, n_frames, K.DRAW_ROWS, tw, K.DRAW_ROWS, fw, K.DRAW_ROWS, cfw)
                assert mv.size == 4 * K.DRAW_ROWS
                s = K.near_integer_share(mv)
                shares.append(s)
                total += int(round(s * mv.size))
                assert s >= K.NEAR_FLOOR, (n_mels, n_frames, tw, fw, cfw, seed, s)
    print(f"near-integer share per launch: min {min(shares):.2e} max {max(shares):.2e}; spans near a boundary in the sweep: {total}")
    assert max(shares) < 0.01 and total > 300
