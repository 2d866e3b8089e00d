#!/usr/bin/env python3
"""Headline benchmark: QuartzNet15x5 inference, batch 64 x 15 s of 16 kHz audio per GPU, bf16 (BASELINE.json
configs[1]).  One "step" = mel front end -> 78 fused TCS launches -> decoder -> argmax + run-collapse, inputs
resident in HBM, replayed from a hipGraph.

    python bench.py --gpus N --steps K --warmup W          (N > 1 without WORLD_SIZE: starts its own N ranks as child processes)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0.  Inference shards by clip (independent units, no collective on the data path):
every rank runs its own 64-clip batch, scaling is "weak".  The timed steps rotate through 5 distinct 64 x 15 s waveform batches
(307 MB > the 256 MB Infinity Cache), so the front end reads its input from HBM.  A plain run does only what the headline needs: set-up,
warm-up, the timed steps, the outputs of the last step (--dump-outputs DIR) and the line (`metric`, `value`, `unit`, `higher_is_better`,
`dtype`, `ms_per_step`, `config`).

--dump-outputs DIR writes what the last timed step returned on rank 0 -- logits [B, V, T'] (bf16 values, stored as float32), the greedy
decode's ids [B, T'], collapsed ids [B, T'] (zero past each row's count) and counts [B], all as float32 -- to DIR/<name>.npy; the inputs
and weights are seeded, so two builds can be compared output for output.

--full adds everything else the benchmark measures or checks, each taking runs of its own.  `roofline` is for the dominant kernel
family (ts::tcs_split_kernel / ts::tcs_kernel, all 78 launches of a step): algorithmic bytes (ideal fusion) / HIP-event time
of the encoder segment.  `cpu_baseline` times the CPU oracle (a port of the reference path, fp32 torch-CPU ops) on a bounded sample of the same
workload on the host cores: P worker processes x 16 torch threads over disjoint clips, P swept IN THIS RUN (1, 4, 16 where the host has
the cores), best aggregate reported with `processes`, `threads`, `host_cores` (started before this process touches the GPU).  `check`
compares the first 16 clips of the measured batch with the fp32 oracle, `check_trained` does the same on weights trained first, and
`predict_api` times `module.predict()`.  The DDP fine-tuning step (`extra.c4_ddp`) runs on every N; at N = 1 the same JSON object also
carries in `extra` the other BASELINE.json configurations (C3, C4 phases 1 and 2, C5) measured by tools/bench_extra.py in the same
process, each with its own roofline (and oracle check where affordable); --no-extra skips them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_BF16_PEAK_TF = 2500.0   # dense bf16


def pmc_traffic(batch, seconds):
    """HBM-side bytes per TCS launch from the PMC passes of this same workload (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in
    separate runs, gfx950 correction applied; tools/prof_bench.sh writes profiles/*_traffic.json).  Counters cannot be read
    from inside the timed process, so this is the committed measurement; None for any other workload."""
    if (batch, seconds) != (64, 15):
        return None, None
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_traffic.json")))
    if not files:
        return None, None
    with open(files[-1]) as f:
        return json.load(f).get("traffic_bytes_per_launch"), "committed PMC pass, profiles/" + os.path.basename(files[-1])


def build_model(device, seed=0):
    from thunder_speech_amd.quartznet.compatibility import build_synthetic_quartznet
    from thunder_speech_amd.utils import variance_preserving_init_
    module = build_synthetic_quartznet(repeat_blocks=3)
    variance_preserving_init_(module.encoder, module.decoder, seed=seed)
    return module.to(device).eval()


def encoder_layers(module):
    layers = []
    for blk in module.encoder:
        layers.extend(blk._cache.get(blk._params(), blk._compile))
    return layers


def cpu_baseline_sweep(seconds=15, budget_s=40.0, repeat_blocks=3):
    """`cpu_baseline`, measured in this run: the oracle (port of the reference path, fp32 torch-CPU ops) as P processes x T threads over
    disjoint clips of the workload (tools/cpu_oracle_worker.py), P swept over (1, 4, 16) as far as the host has P * T cores (T = 16, where one
    torch-CPU process peaks for this model: more threads only add synchronisation), plus a 1-process x 1-thread point.  Every
    configuration: the workers build the model, run one warm-up pass, wait at a common start line, run `iters` timed passes; the
    configuration's rate is (all clips x seconds x iters) / (the slowest worker's time).  The best rate is the value.  MUST run before this
    process initialises the GPU (the workers are child processes)."""
    import subprocess
    host = os.cpu_count() or 1
    threads = min(16, host)
    t_start = time.perf_counter()
    worker = os.path.join(ROOT, "tools", "cpu_oracle_worker.py")
    points = []

    def run_config(procs, thr, clips_each, iters):
        env = dict(os.environ, OMP_NUM_THREADS=str(thr), MKL_NUM_THREADS=str(thr))
        ps = [subprocess.Popen([sys.executable, worker, "--first", str(i * clips_each), "--clips", str(clips_each), "--threads", str(thr),
                                "--iters", str(iters), "--seconds", str(seconds), "--repeat-blocks", str(repeat_blocks)],
                               stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env) for i in range(procs)]
        try:
            for p in ps:
                line = p.stdout.readline().strip()
                if line != "READY":
                    raise RuntimeError(f"cpu_oracle_worker said {line!r}")
            for p in ps:                                  # common start line
                p.stdin.write("GO\n")
                p.stdin.flush()
            res = [json.loads(p.stdout.readline()) for p in ps]
            for p in ps:
                p.wait(timeout=30)
        finally:
            for p in ps:
                if p.poll() is None:
                    p.kill()                              # the exact processes this call started
        slowest = max(r["seconds"] for r in res)
        return {"processes": procs, "threads": thr, "clips_per_process": clips_each, "iters": iters,
                "value": procs * clips_each * seconds * iters / slowest, "slowest_worker_s": slowest}

    for procs in (1, 4, 16):
        if procs > 1 and procs * threads > host:
            break
        if time.perf_counter() - t_start > 0.7 * budget_s:
            break
        good_so_far = [p for p in points if "value" in p]
        if len(good_so_far) >= 2 and good_so_far[-1]["value"] < 1.25 * good_so_far[-2]["value"]:
            # four times the processes did not even buy 25 %: the host is out of memory bandwidth (or of CPU quota), sixteen would only cost the
            # run another ~25 s (measured on the pool's boxes: 243 / 185 / 66 audio-s/s at 1 / 4 / 16 processes) -- recorded as skipped
            points.append({"processes": procs, "threads": threads, "skipped": "the previous step of the sweep scaled by less than 1.25x"})
            break
        try:
            points.append(run_config(procs, threads, max(2, 16 // procs), 3))
        except Exception as e:                            # noqa: BLE001 -- recorded; the headline line must still come out
            points.append({"processes": procs, "threads": threads, "error": f"{type(e).__name__}: {e}"})
    one = None
    if time.perf_counter() - t_start < 0.8 * budget_s:
        try:
            one = run_config(1, 1, 2, 1)
        except Exception as e:                            # noqa: BLE001
            one = {"error": f"{type(e).__name__}: {e}"}
    good = [p for p in points if "value" in p]
    if not good:
        return {"error": "no CPU configuration finished", "sweep": points}
    best = max(good, key=lambda p: p["value"])
    return {"value": best["value"], "unit": "audio-seconds/s", "cores": best["processes"] * best["threads"], "processes": best["processes"],
            "threads": best["threads"], "host_cores": host, "kind": "port",
            "sample": f"QuartzNet15x5 fp32 oracle, {best['processes']} process(es) x {best['threads']} threads, {best['clips_per_process']} x {seconds} s clips each "
                      f"(disjoint clips of the workload), {best['iters']} timed passes after 1 warm-up, common start line",
            "sweep": points, "one_thread": one, "measured_in_this_run": True, "sweep_wall_s": round(time.perf_counter() - t_start, 1)}


def oracle_logits(module, wav, seconds, threads=16):
    """fp32 oracle logits [n, V, T'] of `wav` (CPU): the checker of the headline configuration's full-size parity statement."""
    from oracle import frontend as ofe
    from oracle import tcs as otcs
    torch.set_num_threads(max(1, min(threads, os.cpu_count() or 1)))
    arch = otcs.quartznet_arch(repeat_blocks=3)
    sd = {k: v.detach().cpu() for k, v in module.encoder.state_dict().items()}
    dsd = {k: v.detach().cpu() for k, v in module.decoder.state_dict().items()}
    lengths = torch.full((wav.shape[0],), 16000 * seconds)
    with torch.no_grad():
        feats, fl = ofe.filterbank_features(wav, lengths)
        enc, _ = otcs.encoder_forward(arch, sd, feats, fl)
        return otcs.conv1d_decoder_forward(dsd, enc)


def predict_api(module, wavs, batch, seconds, headline_value):
    """What a drop-in user gets: wall time of `module.predict(wav)` (reference module.py:88-100) per call -- input copy into the module's
    replayed graph, the ~90 launches, D2H of the collapsed ids and the host string join included -- with the module's inference graph on
    (the default) and off (eager launches from Python), at the headline size (C2) and at C1's named size (QuartzNet5x5, 4 x 10 s)."""
    from thunder_speech_amd.quartznet.compatibility import build_synthetic_quartznet
    from thunder_speech_amd.utils import variance_preserving_init_

    def timed(mod, inputs, n):
        for i in range(3 * len(inputs)):          # every input buffer is seen three times: its (zero-copy) graph exists before the clock starts
            strings = mod.predict(inputs[i % len(inputs)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            strings = mod.predict(inputs[i % len(inputs)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, strings

    def both(mod, inputs, n, audio_s):
        res = {}
        for tag, flag in (("graph_on", None), ("graph_off", False)):
            mod.graph_inference = flag
            mod.reset_inference_graphs()
            dt, strings = timed(mod, inputs, n)
            res[tag] = {"ms_per_call": dt * 1e3, "audio_seconds_per_s": audio_s / dt, "mean_chars_per_string": sum(map(len, strings)) / len(strings)}
        return res

    out = {"what": "wall time per module.predict(wav) call incl. the D2H of the collapsed ids and the host string join; graph_on = the module's own "
                   "hipGraphs (default in eval mode under no_grad; zero-copy: keyed by the input buffer's address), graph_off = eager launches from "
                   "Python; inputs rotate through the headline's 5 buffers"}
    with torch.no_grad():
        dev = wavs[0].device
        c2 = both(module, wavs, 20, batch * seconds)
        c2["workload"] = f"QuartzNet15x5, {batch}x{seconds} s (BASELINE.json configs[1])"
        c2["graph_on_vs_headline"] = c2["graph_on"]["audio_seconds_per_s"] / headline_value
        out["c2"] = c2
        m5 = build_synthetic_quartznet(repeat_blocks=1)
        variance_preserving_init_(m5.encoder, m5.decoder, seed=0)
        m5 = m5.to(dev).eval()
        g = torch.Generator().manual_seed(77)
        w5 = [(0.1 * torch.randn(4, 160000, generator=g)).to(dev) for _ in range(3)]
        c1 = both(m5, w5, 50, 40.0)
        c1["workload"] = "QuartzNet5x5, 4x10 s (BASELINE.json configs[0] at its named size, on the GPU)"
        out["c1"] = c1
    module.graph_inference = False
    module.reset_inference_graphs()
    return out


def scaling_block(result, c4_ddp):
    """Per-N summary for the driver's 1 / 2 / 4 / 8 runs: this run's N, audio-s/s, c4_ddp step/s, and the speed-up against the N = 1 line a
    previous run of this checkout stored (gpurun_out/bench_n1.json; written by every N = 1 run).  Efficiency is the driver's to compute."""
    store = os.path.join(ROOT, "gpurun_out", "bench_n1.json")
    n = result["n_gpus"]
    cur = {"n_gpus": n, "audio_seconds_per_s": result["value"],
           "c4_ddp_step_per_s": (c4_ddp or {}).get("value"), "c4_ddp_ms_per_step": (c4_ddp or {}).get("ms_per_step")}
    blk = dict(cur, inference_scaling="weak (64 x 15 s per GPU)", c4_ddp_scaling="strong (global batch 256 x 10 s)")
    if n == 1:
        try:
            os.makedirs(os.path.dirname(store), exist_ok=True)
            with open(store, "w") as f:
                json.dump(cur, f)
        except OSError:
            pass
        blk["vs_n1"] = {"audio_seconds_per_s": 1.0, "c4_ddp_step_per_s": 1.0 if cur["c4_ddp_step_per_s"] else None, "n1_source": "this run"}
    else:
        try:
            with open(store) as f:
                n1 = json.load(f)
            blk["vs_n1"] = {"audio_seconds_per_s": cur["audio_seconds_per_s"] / n1["audio_seconds_per_s"],
                            "c4_ddp_step_per_s": (cur["c4_ddp_step_per_s"] / n1["c4_ddp_step_per_s"]) if (cur["c4_ddp_step_per_s"] and n1.get("c4_ddp_step_per_s")) else None,
                            "n1_source": "gpurun_out/bench_n1.json (the N = 1 run of this checkout)", "n1": n1}
        except (OSError, ValueError, KeyError, ZeroDivisionError):
            blk["vs_n1"] = None                      # no N = 1 line stored on this box
    return blk


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, outputs):
    """The last timed step's outputs as float32 DIR/<name>.npy (every value is exact in float32: bf16 logits, int32 ids and counts below
    2^24).  A batch whose outputs exceed DUMP_LIMIT_BYTES is cut to its first clips, the same ones in every array."""
    import numpy as np
    names = ("logits", "ids", "collapsed", "counts")
    arrays = [t.float().cpu().numpy() for t in outputs]
    per_clip = sum(a[0].nbytes for a in arrays)
    keep = max(1, min(arrays[0].shape[0], DUMP_LIMIT_BYTES // per_clip))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in zip(names, arrays):
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(a[:keep]))


def parity_check(gpu_logits, ref_logits, gpu_ids, labels_blank=28):
    """HIP logits [n, V, T'] (bf16 activations) vs the fp32 oracle's on the same clips: error relative to the logit scale, argmax
    agreement on the frames the oracle decides by more than 6 sigma of the measured error, and the greedy strings of those clips
    (strings are compared on the decided frames' collapse: a near-tie frame may legitimately flip under bf16 rounding)."""
    import numpy as np
    got = gpu_logits.float().cpu().numpy()
    ref = ref_logits.float().numpy()
    scale = float(np.abs(ref).max())
    err = got - ref
    rms = float(np.sqrt(np.mean(err.astype(np.float64) ** 2)))
    top2 = np.sort(ref, axis=1)[:, -2:, :]
    decided = (top2[:, 1] - top2[:, 0]) > 6 * rms
    a_got, a_ref = got.argmax(1), ref.argmax(1)
    agree_decided = bool(np.array_equal(a_got[decided], a_ref[decided]))
    return {"vs": f"fp32 oracle logits on the first {got.shape[0]} clips of the batch, all {got.shape[2]} frames",
            "max_err_over_scale": float(np.abs(err).max()) / scale, "rms_err_over_scale": rms / scale, "logit_scale": scale,
            "decided_frames_frac": float(decided.mean()), "argmax_equal_on_decided_frames": agree_decided,
            "argmax_equal_all_frames_frac": float((a_got == a_ref).mean()),
            "device_argmax_equals_host_argmax_of_device_logits": bool(np.array_equal(gpu_ids, a_got)), "finite": bool(np.isfinite(got).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=15)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the C3 / C4 / C5 measurements (extra.*)")
    ap.add_argument("--extra", default="c3,c4,c5,c5_finetune", help="which of c3,c4,c5,c5_finetune to measure at N = 1")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly from Python instead of replaying a hipGraph")
    ap.add_argument("--weights", choices=("random", "trained"), default="random",
                    help="random: random-init weights of the architecture (the contract's default); trained: QuartzNet15x5 trained on this box first "
                         "(tools/train_margin_model.py, ~1 min) -- timing is the same, `check` then compares transcripts that mean something")
    ap.add_argument("--no-trained-check", action="store_true", help="skip `check_trained` (training on the box + transcript identity vs the fp32 oracle)")
    ap.add_argument("--no-predict-api", action="store_true", help="skip `predict_api` (module.predict() wall time, graph on / off, C2 and C1 sizes)")
    ap.add_argument("--input-batches", type=int, default=5, help="distinct waveform batches the timed steps rotate through (5 x 61 MB > the 256 MB Infinity Cache)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline, cpu_baseline, check, check_trained, predict_api, extra, scaling_block")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step (rank 0) to DIR/<name>.npy as float32")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # one command starts all ranks (the reference: Trainer(accelerator="gpu", devices=-1)): nothing above has touched the GPU, so start
        # one CHILD process per GPU under torch.distributed.run, relay rank 0's line (inherited stdout) and leave with the launcher's code
        from thunder_speech_amd.parallel import launch_ranks
        rc = launch_ranks(os.path.abspath(__file__), args.gpus, sys.argv[1:], timeout_s=float(os.environ.get("TS_BENCH_LAUNCH_TIMEOUT_S", "1500")))
        if rc != 0:
            print(f"bench.py: the {args.gpus}-rank run failed (launcher exit code {rc})", file=sys.stderr)
        sys.exit(rc)
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    # the CPU baseline runs FIRST: its worker processes are children of a process that has not touched the GPU yet
    cpu_sweep = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_sweep = cpu_baseline_sweep(seconds=args.seconds)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible (this benchmark has no CPU path)", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    # launched by torch.distributed.run (WORLD_SIZE set) -- with ANY number of ranks, one included -- the RCCL group comes up and every
    # collective of the multi-rank path runs (probe all-reduce, barriers, max-over-ranks, the gradient exchange of c4_ddp)
    dist_on = "WORLD_SIZE" in os.environ
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        probe = torch.ones(1, device=device)
        dist.all_reduce(probe)                      # a real RCCL all-reduce: its sum IS the number of ranks that took part
        rccl_world = int(probe.item())
        if rccl_world != dist.get_world_size():
            raise RuntimeError(f"RCCL all-reduce saw {rccl_world} ranks, expected {dist.get_world_size()}")
    else:
        rccl_world = 1

    from thunder_speech_amd.module import greedy_decode
    from thunder_speech_amd.parallel import max_over_ranks
    from thunder_speech_amd.utils import tcs_algorithmic_bytes
    B, S = args.batch, args.seconds
    trained_info = None
    if args.weights == "trained":
        from tools import train_margin_model as tmm
        t_tr = time.perf_counter()
        module, hist = tmm.train(device, verbose=False)
        trained_info = {"train_seconds": time.perf_counter() - t_tr, "ctc_loss_first_last": [hist[0][1], hist[-1][1]], "steps": hist[-1][0] + 1,
                        "validation_margin": hist[-1][2]}
        wavs = [tmm.tone_clips(B, S, 4242 + rank + 1000 * i, "cpu")[0].to(device) for i in range(max(args.input_batches, 1))]   # the task's own clips
    else:
        module = build_model(device)
        g = torch.Generator().manual_seed(1234 + rank)
        wavs = [(0.1 * torch.randn(B, 16000 * S, generator=g)).to(device) for _ in range(max(args.input_batches, 1))]
    # the timed steps rotate through `wavs`: 5 x 61.4 MB of distinct samples do not fit the 256 MB Infinity Cache, so every step's front end
    # reads its waveforms from HBM (one replayed graph per input buffer: no copy inside the timed region)
    wav = wavs[0]
    lengths = torch.full((B,), 16000 * S, dtype=torch.int32, device=device)
    module.graph_inference = False          # the headline times the launch sequence under bench.py's own graphs; `predict_api` below times the module's

    def step(w=None):
        logits, _ = module(wav if w is None else w, lengths)
        return (logits,) + tuple(greedy_decode(logits))

    def encoder_only(feats, fl):
        return module.encoder(feats, fl)

    with torch.no_grad():
        for _ in range(2):          # eager warm-up: packs weights, sizes the allocator, sets kernel attributes
            out = step()
        torch.cuda.synchronize()
        if args.full:
            feats, fl = module.audio_transform(wav, lengths)
        side = torch.cuda.Stream(device)
        if args.no_graph:
            run_steps = [(lambda w=w: step(w)) for w in wavs]
            run_enc = lambda: encoder_only(feats, fl)
        else:
            g_steps, outs = [torch.cuda.CUDAGraph() for _ in wavs], []
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):
                step()                          # the library's arena buffers are per stream: let this stream's exist (and be zeroed once)
                if args.full:
                    encoder_only(feats, fl)     # before the capture, or their one-time zero fill would be replayed with every step
                for gs_, w in zip(g_steps, wavs):
                    with torch.cuda.graph(gs_, stream=side):
                        outs.append(step(w))
                if args.full:
                    g_enc = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g_enc, stream=side):
                        enc_out = encoder_only(feats, fl)
                    run_enc = g_enc.replay
            run_steps = [gs_.replay for gs_ in g_steps]
        n_in = len(run_steps)

        def barrier():
            if dist_on:
                dist.barrier()

        from tools import prof_mark
        for i in range(args.warmup):
            run_steps[i % n_in]()
        barrier(); torch.cuda.synchronize()
        prof_mark.mark(device)                      # profiled runs (TS_PROF_MARK=1): brackets the timed region in the kernel trace
        t0 = time.perf_counter()
        for i in range(args.steps):
            out = run_steps[i % n_in]()
        torch.cuda.synchronize(); barrier()
        dt = time.perf_counter() - t0
        prof_mark.mark(device)
        dt = max_over_ranks(dt, device, force=dist_on)
        if args.dump_outputs and rank == 0:
            # before anything else runs on the device: the last step's outputs may live in the library's per-stream arena
            dump_outputs(args.dump_outputs, out if args.no_graph else outs[(args.steps - 1) % n_in])

        if args.full:
            # dominant kernel family: the fused TCS launches of the encoder, timed with HIP events on the launch stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            run_enc(); torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                run_enc()
            e1.record(); torch.cuda.synchronize()
            enc_ms = e0.elapsed_time(e1) / args.steps

    value = world * B * S * args.steps / dt
    result = {
        "metric": "audio-seconds/s (16 kHz) QuartzNet15x5 inference",
        "value": value, "unit": "audio-seconds/s", "n_gpus": world, "rccl_world_size": rccl_world,
        "process_group": "nccl (RCCL), size from a real all-reduce" if dist_on else None, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16", "data": "synthetic",
        "config": {"workload": f"QuartzNet15x5 inference, batch {B}x{S} s per GPU, 16 kHz synthetic clips "
                               "(BASELINE.json configs[1]); step = mel front end + 78 fused TCS launches + decoder + "
                               "greedy decode (argmax + collapse), hipGraph replay" if not args.no_graph else
                               f"QuartzNet15x5 inference, batch {B}x{S} s per GPU (eager launches)",
                   "input_batches_rotated": len(wavs), "input_bytes_rotated": len(wavs) * B * 16000 * S * 4,
                   "batch_per_gpu": B, "clip_seconds": S, "random_init": args.weights == "random", "weights": args.weights, "trained": trained_info},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(result), flush=True)
        if dist_on:
            dist.barrier()
            dist.destroy_process_group()
        return
    layers = encoder_layers(module)
    n_frames = 16000 * S // 160 + 1
    alg_bytes, alg_flops, _ = tcs_algorithmic_bytes(layers, B, n_frames)
    n_launch = len(layers)
    achieved = alg_bytes / (enc_ms * 1e-3) / 1e9
    traffic, traffic_source = pmc_traffic(B, S)
    result["roofline"] = {"bound": "hbm", "kernel": "ts::tcs_split_kernel / ts::tcs_kernel (all fused TCS launches of one step)",
                          "launches_per_step": n_launch,
                          "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                          "traffic": traffic, "traffic_source": traffic_source,
                          "algorithmic_bytes_per_launch": alg_bytes / n_launch, "avg_launch_us": enc_ms * 1e3 / n_launch,
                          "encoder_ms": enc_ms, "mfma_tflops": alg_flops / (enc_ms * 1e-3) / 1e12,
                          "mfma_frac_of_dense_bf16_peak": alg_flops / (enc_ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TF}
    if rank == 0:
        if not args.no_cpu_baseline and world == 1:
            n_chk = min(16, B)
            result["cpu_baseline"] = cpu_sweep
            ref_logits = oracle_logits(module, wav[:n_chk].cpu(), S)      # the checker: fp32 oracle on the first clips of the GPU batch
            with torch.no_grad():
                logits, _ = module(wav, lengths)
                ids, collapsed, counts = greedy_decode(logits)
                torch.cuda.synchronize()
            result["check"] = parity_check(logits[:n_chk], ref_logits, ids[:n_chk].cpu().numpy())
            from oracle import decode as odec
            ref_seqs = [list(odec.collapse_repeats(r)) for r in ref_logits.argmax(1).numpy()]
            dev_seqs = [collapsed[i, : int(counts[i])].cpu().tolist() for i in range(n_chk)]
            result["check"]["collapsed_sequences_equal"] = sum(int(a == b) for a, b in zip(ref_seqs, dev_seqs))
            result["check"]["collapsed_sequences_compared"] = n_chk
            result["check"]["all_logits_finite"] = bool(torch.isfinite(logits).all())
            if not args.no_trained_check:
                # the transcript clause of north_star at this configuration's size, on weights that transcribe: QuartzNet15x5 trained on this box
                # by the repository's own graphed CTC step (tools/train_margin_model.py), then HIP bf16 inference vs the fp32 oracle on 16 of
                # 64 x 15 s clips -- collapsed label sequences, strings and every frame's argmax
                try:
                    from tools import train_margin_model as tmm
                    if args.weights == "trained":
                        m_tr, info = module, dict(trained_info)
                    else:
                        t_tr = time.perf_counter()
                        m_tr, hist = tmm.train(device, verbose=False)
                        info = {"train_seconds": time.perf_counter() - t_tr, "ctc_loss_first_last": [hist[0][1], hist[-1][1]], "steps": hist[-1][0] + 1,
                        "validation_margin": hist[-1][2]}
                    result["check_trained"] = dict(tmm.evaluate(m_tr, device, batch=B, seconds=S, n_check=n_chk), train=info)
                    del m_tr
                except Exception as e:                    # noqa: BLE001 -- recorded; the headline line must still come out
                    import traceback
                    print(f"bench.py: check_trained failed:\n{traceback.format_exc()}", file=sys.stderr, flush=True)
                    result["check_trained"] = {"error": f"{type(e).__name__}: {e}"}
    if rank == 0 and world == 1 and not args.no_predict_api:
        try:
            result["predict_api"] = predict_api(module, wavs, B, S, value)
        except Exception as e:                            # noqa: BLE001 -- recorded; the headline line must still come out
            import traceback
            print(f"bench.py: predict_api failed:\n{traceback.format_exc()}", file=sys.stderr, flush=True)
            result["predict_api"] = {"error": f"{type(e).__name__}: {e}"}
    # C4 as the reference runs it (DDP, strong scaling: global batch 256 x 10 s over the ranks), on EVERY N: all ranks take part.
    # An extra must never take the headline line down with it: exceptions are recorded, and a watchdog on every rank covers what an
    # exception handler cannot -- a collective that never returns (e.g. because ONE rank failed): past the deadline rank 0 prints the
    # line with the error in place of the result and every rank leaves.
    c4_ddp = None
    failed_extra = False
    extras = [n for n in args.extra.split(",") if n]
    if not args.no_extra and ("c4" in extras or "c4_ddp" in extras):
        del module
        module = None
        torch.cuda.empty_cache()
        import threading
        deadline = float(os.environ.get("TS_BENCH_EXTRA_DEADLINE_S", "240"))

        def give_up():
            # watchdog: a collective never returned (e.g. ONE rank failed).  Every rank says so on stderr and leaves with a NON-ZERO code (the
            # launcher must see the failure); rank 0 flushes the headline line first, with the error in place of the result.
            print(f"bench.py rank {rank}: extra c4_ddp gave no result within {deadline:.0f} s -- giving up", file=sys.stderr, flush=True)
            if rank == 0:
                result.setdefault("extra", {})["c4_ddp"] = {"error": f"no result within {deadline:.0f} s (a rank failed or a collective did not return)"}
                print(json.dumps(result), flush=True)
            os._exit(3)

        dog = threading.Timer(deadline, give_up)
        dog.daemon = True
        dog.start()
        from tools import bench_extra
        try:
            c4_ddp = bench_extra.c4_ddp(device, world=world, rank=rank)
            if dist_on:
                dist.barrier()                       # every rank got through: only now is it safe to stop the watchdogs
        except Exception as e:
            import traceback
            print(f"bench.py rank {rank}: extra c4_ddp failed:\n{traceback.format_exc()}", file=sys.stderr, flush=True)
            c4_ddp = {"error": f"{type(e).__name__}: {e}"}
            if world > 1:                            # the other ranks may be waiting in a collective this rank will never enter:
                if rank == 0:                        # leave now (never re-exec), non-zero, after rank 0 has flushed the headline line
                    result.setdefault("extra", {})["c4_ddp"] = c4_ddp
                    print(json.dumps(result), flush=True)
                os._exit(3)
            failed_extra = True
        dog.cancel()
        torch.cuda.empty_cache()
    if rank == 0:
        if not args.no_extra and world == 1:
            from tools import bench_extra
            result["extra"] = bench_extra.run(device, tuple(n for n in extras if n != "c4_ddp"), check=not args.no_cpu_baseline)
            failed_extra = failed_extra or any(isinstance(v, dict) and "error" in v for v in result["extra"].values())
        if c4_ddp is not None:
            result.setdefault("extra", {})["c4_ddp"] = c4_ddp
        result["scaling_block"] = scaling_block(result, c4_ddp)
        print(json.dumps(result), flush=True)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()
    if failed_extra:
        sys.exit(3)                                  # the line above is complete, but an extra failed: the launcher must see it


if __name__ == "__main__":
    main()
