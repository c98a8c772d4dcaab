#!/usr/bin/env python3
"""Headline benchmark: NPPC K=5 FullSubNet+ train step, spectrogram-frames/s on MI355X.

  python bench.py --gpus N --steps K --warmup W [--config c2|c3|c5] [--dump-outputs DIR] [--full]

A plain run does only what the headline figure needs: set up, warm up, time the K steps, write --dump-outputs, print the
line.  --full adds what takes runs of its own, after the timed steps (one GPU): the untimed per-launch pass that ranks every
kernel and times the HBM-bound families, the fp32 parity-mode steps and the CPU baseline (--no-families, --no-fp32 and
--no-cpu-baseline leave one of them out).

N > 1 without an external launcher: bench.py starts its own N ranks (`python -m torch.distributed.run ... bench.py`) as a
CHILD process before anything touches the GPU and exits with the child's code; under an external torch.distributed.run
(WORLD_SIZE set) it is a rank.

One "step" (c2, the default = BASELINE config 2; c5 = config 5: 8 x 30 s, K=8) = one full train step on one minibatch
of synthetic 16 kHz noisy speech that is already resident in HBM: noisy+clean STFT, frozen FullSubNet+ restorer
forward, cIRM build/apply, K-direction net forward, Gram-Schmidt, NPPC loss, full backward, gradient all-reduce
(N > 1), Adam.  Weak scaling: every rank runs the per-GPU batch, rank r on clips [B*r, B*r+B).  Weights: seeded random
init (no checkpoint offline).  --config c3 = BASELINE config 3 (inpainting sibling, single GPU), same JSON schema.
Prints ONE JSON line on rank 0; ms_per_step = wall time of the K timed steps / K.  --dump-outputs DIR writes what the last
timed step computed (its returned arrays and the direction net's updated parameters) as DIR/<name>.npy, <= 64 MB in all,
for output-for-output comparison of two builds: inputs and initial weights are seeded, identical from run to run.

What the line's extra objects mean (definitions and byte/FLOP counts: DESIGN.md section 4):
  roofline        the kernel with the largest total duration per step (--full: HIP events around every launch in an
                  untimed pass rank the kernels; otherwise only the LSTM launches of the timed region are ranked, as
                  `ranked_over` says; `achieved` of an LSTM kernel comes from HIP events inside the TIMED region);
                  on a < 1 % tie the lower fraction is reported.  roofline.step = whole-step algorithmic FLOP rate.
  roofline.hbm_families   (--full) achieved GB/s of the HBM-bound kernel families = algorithmic bytes / HIP-event time
  fp32            (--full) the precision-matched (reference dtype) step time, a few steps outside the timed region
  cpu_baseline    (--full) the oracle (CPU restatement pinned to the reference by tests/golden) on a bounded sample
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "generative-audio_amd"))

BATCH, SECONDS, SR, K_DIRS = 32, 4, 16000, 5
NFFT, HOP, NF = 512, 256, 257
PEAK_BF16_TFLOPS = 2500.0     # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3       # fp32 matrix (= vector) peak
PEAK_HBM_GBS = 8000.0
PMC_CSV = os.path.join(ROOT, "profiles", "r04_bench_c2_bf16_pmc_traffic.csv")
PMC_STAMP = os.path.join(ROOT, "profiles", "r04_bench_c2_bf16_pmc_stamp.json")
PMC_C5 = (os.path.join(ROOT, "profiles", "r04_bench_c5_bf16_pmc_traffic.csv"), os.path.join(ROOT, "profiles", "r04_bench_c5_bf16_pmc_stamp.json"))


def build_trainer(precision, rank, world, batch, length, n_dirs=K_DIRS):
    from nppc_audio.data import SyntheticNoisySpeech
    from nppc_audio.fullsubnet import FullSubNet_Plus, FullSubNetPlusConfig
    from nppc_audio.trainer import NPPCAudioTrainer, NPPCAudioTrainerConfig
    torch.manual_seed(0)                                         # identical init on every rank
    rest_cfg = dict(num_groups_in_drop_band=1, precision=precision)
    tmp = tempfile.mkdtemp(prefix=f"nppc_bench_r{rank}_")
    ck = os.path.join(tmp, "restorer.tar")
    torch.save({"model": FullSubNet_Plus(FullSubNetPlusConfig(**rest_cfg)).state_dict()}, ck)
    cfg = NPPCAudioTrainerConfig(
        nppc_model_configuration=dict(
            pretrained_restoration_model_configuration=rest_cfg, pretrained_restoration_model_path=ck,
            audio_pc_wrapper_configuration=dict(multi_direction_configuration=dict(
                num_groups_in_drop_band=2, n_directions=n_dirs, precision=precision)),
            stft_configuration=dict(nfft=NFFT, hop_length=HOP, win_length=NFFT), device="cuda"),
        data_configuration=dict(data_path=".", dataset=dict(clean_path=".", noisy_path=".")),
        data_loader_configuration=dict(batch_size=batch * world, num_workers=0, pin_memory=False, shuffle=False),
        optimizer_configuration=dict(type="Adam", args=dict(lr=1e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=0)),
        device="cuda")
    ds = SyntheticNoisySpeech(batch * world, length)
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):          # the trainer prints like the reference; stdout is ONE JSON line
        tr = NPPCAudioTrainer(cfg, dataset=ds)
    dev = torch.device("cuda", torch.cuda.current_device())
    # this rank's shard of the (single) global minibatch, uploaded once: inputs are HBM-resident for the timed region
    clips = [ds[rank * batch + i] for i in range(batch)]
    noisy = torch.stack([c[0] for c in clips]).to(dev)
    clean = torch.stack([c[1] for c in clips]).to(dev)
    return tr, (noisy, clean)


def host_cores():
    """CPU threads this process may really use: affinity mask, capped at the GPU box's per-GPU share (16)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def kernel_source_hash(files=None):
    """identifies the kernel sources of the running tree (the GPU box has no .git): sha256 over csrc + the C header, or
    over the listed files of csrc (the translation unit of one kernel: a PMC stamp names the files it covers)"""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "generative-audio_amd", "csrc")
    for f in (sorted(os.listdir(csrc)) if files is None else sorted(files)) + ["../../include/nppc_hip.h"]:
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(rocprof_pattern, workload, PMC_CSV=None, PMC_STAMP=None, expect="C2", aggregate=False):
    """HBM bytes per launch of a kernel (FETCH_SIZE x2 per the gfx950 note + WRITE_SIZE) from the committed rocprofv3
    counter passes of this same command (tools/summarize_pmc.py; counters cannot be collected from inside the timed
    process).  The passes are stamped with the hash of the kernel sources they profiled: a different running tree, a
    different workload or a missing file gives null."""
    import csv
    PMC_CSV, PMC_STAMP = PMC_CSV or globals()["PMC_CSV"], PMC_STAMP or globals()["PMC_STAMP"]
    if workload != expect or rocprof_pattern is None or not (os.path.exists(PMC_CSV) and os.path.exists(PMC_STAMP)):
        return None, "no committed PMC pass for this kernel / configuration"
    stamp = json.load(open(PMC_STAMP))
    now = kernel_source_hash(stamp.get("files"))
    if stamp.get("kernel_source_hash") != now:
        return None, (f"committed PMC pass profiled kernel sources {stamp.get('kernel_source_hash')} (git {stamp.get('git_head')}), "
                      f"the running tree is {now}: stale, not reported")
    note = (f"bytes per launch, {os.path.relpath(PMC_CSV, ROOT)} (separate --pmc passes, git {stamp.get('git_head')}, "
            f"kernel sources {stamp.get('kernel_source_hash')})")
    tot, n = 0.0, 0
    with open(PMC_CSV) as f:
        for r in csv.DictReader(f):
            if rocprof_pattern in r["kernel"]:
                mb = float(r["fetch_MB_per_launch_x2_corrected"]) + float(r["write_MB_per_launch"])
                if not aggregate:
                    return mb * 1048576.0, note
                tot, n = tot + mb * 1048576.0 * int(r["launches"]), n + int(r["launches"])
    if n:           # a family served by several template instantiations of one kernel: launch-weighted mean
        return tot / n, note + f"; mean over the {n} profiled launches of every '{rocprof_pattern}' instantiation"
    return None, "kernel not in the committed PMC summary"


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline():
    """CPU path = the oracle restatement (pinned to the reference by tests/golden) on the METRIC's configuration (SURVEY 8d,
    VERDICT r03 item 8): B = 32 x 4 s (the whole C2 batch), K = 5, G_pc = 2, fp32, full train steps (forward + backward +
    Adam) on the host cores of the GPU box.  Two rows: "reference-shaped" (restorer executed twice and
    the noisy STFT three times per step, exactly as the reference does) -- the `value` -- and "de-duplicated".  One warm-up
    step at full size (reference-shaped), then ONE timed step per row (~30 s each on 16 threads)."""
    sys.path.insert(0, ROOT)
    from oracle import nppc_ref as R
    from oracle import weights as W
    torch.set_num_threads(host_cores())
    B, L = int(os.environ.get("NPPC_BENCH_CPU_BATCH", BATCH)), SECONDS * SR
    spec = W.nppc_spec(K_DIRS)
    P = {k: torch.from_numpy(v) for k, v in W.make_weights(spec, 7).items()}
    train = {k: v.requires_grad_(True) for k, v in P.items() if k.startswith("audio_pc_wrapper")}
    noisy, clean = (torch.from_numpy(a) for a in W.synth_batch(B, L))
    state = {}

    def one(step, n, c, shaped):
        _, obj, _ = R.nppc_step(n, c, P, K_DIRS, step, g_rest=1, g_pc=2, reference_shaped=shaped)
        names = list(train)
        gs = torch.autograd.grad(obj, [train[k] for k in names])
        with torch.no_grad():
            R.adam_step(train, dict(zip(names, gs)), state, step + 1)

    t0 = time.perf_counter()
    one(0, noisy, clean, True)                                # warm-up at full size: thread pool, allocator, MKLDNN primitives
    warm = time.perf_counter() - t0
    frames = B * (1 + L // HOP)
    rows = {}
    for i, (tag, shaped) in enumerate((("reference_shaped", True), ("deduplicated", False))):
        t0 = time.perf_counter()
        one(1 + i, noisy, clean, shaped)
        dt = time.perf_counter() - t0
        rows[tag] = {"frames_per_s": frames / dt, "s_per_step": dt}
    return {"value": rows["reference_shaped"]["frames_per_s"], "unit": "frames/s", "cores": torch.get_num_threads(),
            "kind": "port", "cpu_model": cpu_model(), "rows": rows,
            "sample": f"the metric's own configuration: B={B} x {SECONDS} s, K={K_DIRS}, G_pc=2, fp32; 1 warm-up step ({warm:.1f} s) + 1 timed "
                      f"train step per row; value = reference-shaped row (2x restorer, 3x STFT: "
                      f"{rows['reference_shaped']['s_per_step']:.1f} s/step), de-duplicated row {rows['deduplicated']['s_per_step']:.1f} s/step"}


# ------------------------------------------------------------------------------------------------ algorithmic work
LSTM_FLOP_PER_SEQ_STEP = 2 * 4 * 384 * (34 + 384) + 2 * 4 * 384 * (2 * 384)        # both layers' gate GEMMs


def step_flops(B, T, K, g_pc=2):
    """restorer forward x1 + direction net forward x3 (forward + 2x for backward)"""
    Tv = T + 2
    fo = NF if (g_pc <= 1 or B == 1) else (NF - NF % g_pc) // g_pc
    tcn = lambda C: 3 * (8 * (2048 * C + 3072) + 2 * C * NF)
    rest = B * NF * Tv * (LSTM_FLOP_PER_SEQ_STEP + 2 * 384 * 2) + B * Tv * tcn(NF)
    pc = B * fo * Tv * (LSTM_FLOP_PER_SEQ_STEP + 2 * 384 * 2 * K) + B * Tv * tcn(2 * NF)
    return rest + 3 * pc


def hbm_family_bytes(B, L, T, K, n_params, act_bytes, g_pc=2):
    """algorithmic bytes per step of the HBM-bound kernel families (TCN element-wise: DESIGN.md section 4)
    -> {family: (bytes, [entry points])}"""
    Tv = T + 2
    fo = NF if (g_pc <= 1 or B == 1) else (NF - NF % g_pc) // g_pc
    m = B * NF * T * 4                                 # one fp32 spectrogram map
    W = B * K * 2 * fo * T * 4                         # the K directions
    E = B * 2 * fo * T * 4                             # one cIRM in drop-band order
    act = 3 * B * Tv * 512 * act_bytes                 # one hidden TCN activation, three branches
    return {
        "stft": (2 * B * L * 4 + 5 * m, ["nppc_stft"]),
        "cirm_build_compress": (6 * m, ["nppc_cirm_build_compress"]),
        "cirm_decompress_apply": (7 * m, ["nppc_cirm_decompress_apply_conj"]),
        # 4 source maps per net read once (the unfolded tensor is never algorithmic traffic), both nets
        "subband_staging_fwd": (2 * 4 * B * NF * Tv * 4, ["nppc_subband_mean", "nppc_subband_stage"]),
        "gs_and_loss": (5 * W + 3 * E, ["nppc_gram", "nppc_combine", "nppc_gs_solve", "nppc_gs_bwd_solve", "nppc_loss_solve",
                                        "nppc_loss_solve_eps", "nppc_loss_bwd_coef", "nppc_loss_bwd_coef_dev"]),
        "adam": (7 * 4 * n_params, ["nppc_adam_step"]),
        # per TCN block: forward reads the 1x1-conv output once and writes the depthwise output once (both nets);
        # backward reads the upstream gradient + the two saved activations and writes one gradient (direction net)
        "tcn_elementwise": (8 * (2 * 2 * act + 4 * act), ["nppc_tcn_dwconv", "nppc_tcn_gn_apply", "nppc_tcn_gn_bwd",
                                                          "nppc_tcn_dwconv_bwd", "nppc_tcn_mid_fwd", "nppc_tcn_mid_bwd",
                                                          "nppc_tcn_mid_bwd_reduce"]),
    }


ROCPROF_NAME = {   # bench label prefix -> substring of the rocprofv3 kernel name (template arguments included)
    "lstm2_bwd_coop_ksplit_g4": "lstm2_coop_bwd4_kernel",
    "lstm2_bwd_coop_ksplit": "lstm2_coop_bwd2_kernel",
    "lstm2_fwd_coop_g2[N=8224": "2, 5, 64, false",
    "lstm2_fwd_coop_g2_train[N=4096": "2, 2, 64, true",
    "lstm2_fwd_coop_g4_train": "4, 2, 64, true",
    "lstm2_fwd_ws_train": "lstm2_ws_fwd_kernel<true>",
    "lstm2_fwd_ws": "lstm2_ws_fwd_kernel<false>",
}


DUMP_BUDGET_BYTES = 63_000_000     # --dump-outputs: all .npy payloads together (the files, headers included, stay < 64 MB)
DUMP_SAMPLE_SEED = 20251015        # fixed: two builds sample the same elements of an over-budget array


def step_outputs(step_result, net):
    """what one train step hands its caller -> {name: host tensor}: the returned (reconst_err, objective, log) -- the log's
    echoed inputs left out -- and the direction net's parameters after the step's update (one flat vector, in
    named_parameters() order).  Copied off the device at once: later steps reuse the step-persistent workspaces."""
    reconst_err, objective, log = step_result
    out = {"reconst_err": reconst_err, "objective": objective}
    for k, v in log.items():
        if isinstance(v, torch.Tensor) and k not in ("noisy_complex", "clean_complex", "reconst_err", "objective"):
            out[k] = v
    out["direction_net_params"] = torch.cat([p.detach().reshape(-1).float() for _, p in net.named_parameters()])
    host = {}
    for k, v in out.items():
        v = v.detach()
        if v.is_complex():
            v = torch.view_as_real(v)           # [..., 2] = (real, imag)
        host[k] = v.to("cpu", torch.float64 if v.dtype in (torch.float64, torch.int64, torch.int32) else torch.float32)
    return host


def dump_outputs(dirname, arrays, meta=None):
    """writes arrays {name: host tensor} as dirname/<name>.npy (float32 / float64) within DUMP_BUDGET_BYTES in all.  Arrays
    that fit their share of the budget are written whole; the others as a fixed seeded sample of their flattened elements
    (sorted flat indices, the same for every run of the same shape).  Returns what was written and how, for the JSON line."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    names = sorted(arrays, key=lambda k: (arrays[k].numel() * arrays[k].element_size(), k))
    left = DUMP_BUDGET_BYTES
    manifest = {"dir": os.path.abspath(dirname), "budget_bytes": DUMP_BUDGET_BYTES, "sample_seed": DUMP_SAMPLE_SEED,
                "sampling": "numpy.random.Generator(PCG64(sample_seed)).choice(numel, n, replace=False), sorted, on the "
                            "C-order flattened array", "meta": meta or {}, "arrays": {}}
    for i, k in enumerate(names):
        a = arrays[k].numpy()
        share = left // (len(names) - i)
        entry = {"shape": list(a.shape), "dtype": str(a.dtype), "numel": int(a.size)}
        if a.nbytes > share:
            n = int(share // a.itemsize)
            idx = np.sort(np.random.Generator(np.random.PCG64(DUMP_SAMPLE_SEED)).choice(a.size, n, replace=False))
            a = np.ascontiguousarray(a.reshape(-1)[idx])
            entry["sampled"] = n
        np.save(os.path.join(dirname, k + ".npy"), a)
        left -= a.nbytes
        manifest["arrays"][k] = entry
    log(f"wrote {len(names)} arrays ({(DUMP_BUDGET_BYTES - left) / 1e6:.1f} MB) to {dirname}")
    return manifest


def self_launch(a):
    """--gpus N without an external launcher: start the N ranks as a child torch.distributed.run BEFORE any GPU call of
    this process (a process that initialised the GPU must never exec / must not hold the device the ranks need)"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log(f"starting {a.gpus} ranks: {' '.join(cmd[1:])}")
    return subprocess.call(cmd, env=env)


def dp_selftest(a, world, rank):
    """CPU rehearsal of the launcher + the gradient exchange (gloo): what tests/test_dp_gloo_cpu.py drives"""
    import torch.distributed as dist
    from nppc_audio.dp import FlatGradientReducer
    dist.init_process_group("gloo")
    if a.dp_selftest_fail_rank == rank:
        raise SystemExit(3)
    g = torch.arange(1000, dtype=torch.float32) * (rank + 1)
    red = FlatGradientReducer()
    red.range_ready(g, 700, 1000)
    red.range_ready(g, 100, 300)
    scale = red.finish(g)
    want = torch.arange(1000, dtype=torch.float32) * sum(r + 1 for r in range(world)) / world
    ok = bool(torch.allclose(g * scale, want))
    dist.barrier()
    if rank == 0:
        print(json.dumps({"dp_selftest": ok, "n_gpus": world, "scale": scale}))
    dist.destroy_process_group()
    sys.exit(0 if ok else 4)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "c5"], help="BASELINE.json config (c2 = headline)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--seconds", type=float, default=None)
    ap.add_argument("--dirs", type=int, default=None, help="number of PC directions K")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the per-launch pass, the fp32 steps and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-fp32", action="store_true", help="with --full: skip the precision-matched fp32 steps")
    ap.add_argument("--no-families", action="store_true", help="with --full: skip the per-launch HIP-event pass")
    ap.add_argument("--pipeline", action="store_true", help="pipeline_update mode of the trainer (A/B switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (<= 64 MB in all)")
    ap.add_argument("--dp-selftest", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dp-selftest-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


def extra_passes(a, world):
    """what a run measures beyond its timed steps: nothing without --full; with it, on one GPU, every pass not switched
    off (N > 1: the other ranks have left after the timed steps, more steps would wait for them forever)"""
    on = a.full and world == 1
    return {"families": on and not a.no_families,
            "fp32": on and a.precision == "bf16" and not a.no_fp32,
            "cpu_baseline": on and not a.no_cpu_baseline}


def inpainting_argv(a, extra):
    """--config c3: the command line of tools/bench_inpainting.py, which runs its CPU baseline unless told not to"""
    return (["--steps", str(a.steps), "--warmup", str(a.warmup), "--precision", a.precision]
            + ([] if extra["cpu_baseline"] else ["--no-cpu-baseline"])
            + (["--dump-outputs", a.dump_outputs] if a.dump_outputs else []))


def main():
    a = parse_args()

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if a.dp_selftest:
        return dp_selftest(a, world, rank)
    extra = extra_passes(a, world)
    if a.config == "c3":
        if world > 1:
            raise SystemExit("config c3 (inpainting) is single-GPU: train-mode BatchNorm couples the minibatch (DESIGN.md 8)")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_inpainting
        return bench_inpainting.main(inpainting_argv(a, extra))
    cb, cs, ck = {"c2": (BATCH, SECONDS, K_DIRS), "c5": (8, 30, 8)}[a.config]
    a.batch, a.seconds, a.dirs = a.batch or cb, a.seconds or cs, a.dirs or ck
    workload = {(BATCH, SECONDS, K_DIRS): "C2", (8, 30, 8): "C5"}.get((a.batch, a.seconds, a.dirs), "custom")

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # before the first HIP call: dmabuf IPC for RCCL
    backend = os.environ.get("NPPC_DP_BACKEND", "nccl")           # "gloo": rehearsal of the N > 1 control flow on a 1-GPU box
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    torch.cuda.set_device(local)
    if world > 1:
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            torch.distributed.init_process_group(backend)

    from nppc_audio import _hip as H
    from nppc_audio import ops_lstm
    length = int(a.seconds * SR)
    tr, batch = build_trainer(a.precision, rank, world, a.batch, length, a.dirs)
    T = 1 + length // HOP
    frames = a.batch * T

    def sync():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    if rank == 0:
        log(f"model built; {a.warmup} warm-up + {a.steps} timed steps, {frames} frames/step/GPU")
    tr.pipeline_update = a.pipeline              # park a step's tail in front of the next step's restorer LSTM (no gain on one GPU)
    for _ in range(a.warmup):
        tr.train_step(batch)
    tr.flush()
    sync()
    if rank == 0:
        log("warm-up done")
    ops_lstm.PROFILE = []
    t0 = time.perf_counter()
    for _ in range(a.steps):
        last = tr.train_step(batch)
    tr.flush()                                   # the last step's parked update (weight gradients, exchange, Adam) is inside the timed region
    sync()
    dt = time.perf_counter() - t0
    objective = last[1]
    dumped = step_outputs(last, tr.nppc_model.audio_pc_wrapper.net) if (a.dump_outputs and rank == 0) else None
    del last
    prof, ops_lstm.PROFILE = ops_lstm.PROFILE, None
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda")
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt)
    dp_info = None
    if world > 1:        # what the process group really is: the driver can see that RCCL ran with N ranks
        dp_info = {"world_size": torch.distributed.get_world_size(), "backend": torch.distributed.get_backend(),
                   "nccl_version": ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None,
                   "gradient_exchange": "bucketed inside backward" if tr._reducer.overlap else "one all-reduce behind backward",
                   "pipeline_update": bool(tr.pipeline_update)}
    nto = ops_lstm.coop_timeouts()      # sticky counter: covers every launch since the process started
    if nto:      # a bounded hand-off spin gave up: the step's results are wrong, so is any number measured on them
        raise RuntimeError(f"rank {rank}: {nto} cooperative LSTM hand-off time-outs during the run: measurement invalid")
    if rank != 0:
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    ms_step = 1e3 * dt / a.steps
    log(f"timed region done: {ms_step:.2f} ms/step")
    dump_info = None
    if dumped is not None:
        dump_info = dump_outputs(a.dump_outputs, dumped, meta={"config": a.config, "workload": workload, "precision": a.precision,
                                                   "batch": a.batch, "seconds": a.seconds, "dirs": a.dirs,
                                                   "steps": a.steps, "warmup": a.warmup, "n_gpus": world})
        del dumped

    # ---- LSTM launches inside the timed region (HIP events on the launch stream) --------------------------------
    per = {}
    for label, e0, e1 in prof:
        per.setdefault(label, []).append(e0.elapsed_time(e1))
    kern = {}
    for (name, train, N, Tn, mt), ms in per.items():
        avg = sum(ms) / len(ms)
        lab = f"{name}{'_train' if train and 'fwd' in name else ''}[N={N},T'={Tn},mtile={mt}]"
        kern[lab] = dict(ms=avg, launches_per_step=len(ms) / a.steps, tflops=N * Tn * LSTM_FLOP_PER_SEQ_STEP / (avg * 1e-3) / 1e12)
    peak = PEAK_BF16_TFLOPS if a.precision == "bf16" else PEAK_F32_TFLOPS

    # ---- untimed pass with HIP events around EVERY launch: ranks the kernels, times the HBM-bound families -------
    totals, fam = {}, None
    if extra["families"]:
        NP = 3
        H.PROFILE = []
        for _ in range(NP):
            tr.train_step(batch)
        tr.flush()
        torch.cuda.synchronize()
        calls, H.PROFILE = H.PROFILE, None
        for name, e0, e1 in calls:
            t = totals.setdefault(name, [0.0, 0])
            t[0] += e0.elapsed_time(e1) / NP
            t[1] += 1
        n_params = tr.nppc_model.audio_pc_wrapper.net.engine().fp.flat.numel()
        fam = {}
        for f, (nbytes, names) in hbm_family_bytes(a.batch, length, T, a.dirs, n_params, 2 if a.precision == "bf16" else 4).items():
            ms = sum(totals[n][0] for n in names if n in totals)
            if ms > 0:
                fam[f] = dict(algorithmic_MB=nbytes / 1e6, ms_per_step=ms, launches_per_step=sum(totals[n][1] for n in names if n in totals) / NP,
                              achieved_GBps=nbytes / (ms * 1e-3) / 1e9, frac_of_hbm_peak=nbytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS)
        log(f"per-launch pass done: {sum(v[1] for v in totals.values()) // NP} launches/step")

    # dominant kernel = largest TOTAL duration per step; LSTM launches are told apart by shape (different template
    # instantiations = different kernels in a rocprof summary), everything else by entry point
    rank_ms = {lab: v["ms"] * v["launches_per_step"] for lab, v in kern.items()}
    for name, (ms, _) in totals.items():
        if not name.startswith("nppc_lstm2_") or "pack" in name:
            rank_ms[name] = ms
    ordered = sorted(rank_ms.items(), key=lambda kv: -kv[1])
    dom_name = ordered[0][0] if ordered else "none"
    if len(ordered) > 1 and ordered[1][1] > 0.99 * ordered[0][1] and ordered[0][0] in kern and ordered[1][0] in kern:
        # a < 1 % tie between two LSTM kernels: report the one further from its roofline
        dom_name = min(ordered[:2], key=lambda kv: kern[kv[0]]["tflops"])[0]
    flops_step = step_flops(a.batch, T, a.dirs)
    roof = {"bound": "mfma", "kernel": dom_name, "peak": peak, "unit": "TFLOP/s", "traffic": None,
            "ranked_over": "every launch (untimed per-launch pass)" if totals else "the LSTM launches of the timed region",
            "ranked_ms_per_step": {k: round(v, 3) for k, v in ordered[:12]},
            "all_lstm_kernels": kern,
            "step": {"algorithmic_flop": flops_step, "achieved": flops_step / (ms_step * 1e-3) / 1e12,
                     "frac": flops_step / (ms_step * 1e-3) / 1e12 / peak}}
    if dom_name in kern:
        d = kern[dom_name]
        roof.update(achieved=d["tflops"], frac=d["tflops"] / peak, avg_ms=d["ms"])
        pat = next((v for k, v in ROCPROF_NAME.items() if dom_name.startswith(k)), None)
        if workload == "C5":      # BASELINE config 5 has counter passes of its own
            roof["traffic"], roof["traffic_note"] = pmc_traffic(pat, workload, PMC_C5[0], PMC_C5[1], expect="C5")
        else:
            roof["traffic"], roof["traffic_note"] = pmc_traffic(pat, workload)
    else:
        roof.update(achieved=None, frac=None, avg_ms=rank_ms.get(dom_name))
    if fam is not None:
        roof["hbm_families"] = fam

    out = {
        "metric": f"spectrogram-frames/sec, NPPC K={a.dirs} FullSubNet+ train step",
        "value": world * frames * a.steps / dt,
        "unit": "frames/s",
        "per_gpu": frames * a.steps / dt,
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": ms_step,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16" if a.precision == "bf16" else "f32", "data": "synthetic",
        "config": {"workload": f"{workload}: speech-enhancement NPPC, FullSubNet+ restorer + K={a.dirs} direction net, "
                               f"batch={a.batch}x{a.seconds:g}s@16kHz per GPU, STFT {NFFT}/{HOP}, G_rest=1 G_pc=2, "
                               f"full train step (fwd+loss+bwd+Adam{'+RCCL all-reduce' if world > 1 else ''})",
                   "global_batch": a.batch * world, "frames_per_step_per_gpu": frames,
                   "parallelism": f"dp{world}", "objective_last": float(objective)},
        "roofline": roof,
        "lstm_handoff_timeouts": 0,
    }
    if dp_info is not None:
        out["dp"] = dp_info
    if dump_info is not None:
        out["dumped_outputs"] = dump_info
    if extra["fp32"]:
        # the reference computes in fp32: the same step in the product's fp32 parity mode (exact-f32 MFMA), outside the
        # timed region.  The bf16 trainer's step-persistent workspaces stay allocated (288 GB of HBM: both fit).
        log("timing the fp32 parity mode (1 warm-up + 3 steps)")
        tr32, batch32 = build_trainer("fp32", 0, 1, a.batch, length, a.dirs)
        tr32.pipeline_update = tr.pipeline_update
        tr32.train_step(batch32)
        tr32.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            tr32.train_step(batch32)
        tr32.flush()
        torch.cuda.synchronize()
        ms32 = 1e3 * (time.perf_counter() - t0) / 3
        ops_lstm.check_coop_timeouts("fp32 steps")
        out["fp32"] = {"ms_per_step": ms32, "frames_per_s": frames / (ms32 * 1e-3), "steps": 3,
                       "achieved_tflops": flops_step / (ms32 * 1e-3) / 1e12,
                       "frac_of_fp32_matrix_peak": flops_step / (ms32 * 1e-3) / 1e12 / PEAK_F32_TFLOPS}
        del tr32, batch32
    if extra["cpu_baseline"]:
        log("timing the CPU baseline (bounded sample)")
        out["cpu_baseline"] = cpu_baseline()
        out["gpu_over_cpu"] = out["value"] / out["cpu_baseline"]["value"]
    print(json.dumps(out))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
