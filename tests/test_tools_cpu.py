"""CPU: the measurement helpers bench.py depends on (PMC summary parsing, kernel-name matching) keep working."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(m)
    finally:
        sys.argv = argv
    return m


def test_pmc_traffic_lookup_is_stamped_with_the_profiled_kernel_sources(tmp_path, monkeypatch):
    """roofline.traffic comes from committed rocprofv3 counter passes; it is reported only while the kernel sources of
    the running tree are the ones that were profiled (hash in the stamp file), and only for the profiled workload"""
    import json
    b = _bench()
    csvp, stamp = tmp_path / "t.csv", tmp_path / "s.json"
    csvp.write_text("kernel,launches,FETCH_SIZE_sum_KB,WRITE_SIZE_sum_KB,fetch_MB_per_launch_x2_corrected,write_MB_per_launch\n"
                    '"void lstm2_coop_bwd2_kernel<...>(Args)",13,1,1,1000.0,500.0\n'
                    '"void lstm2_coop_fwd_kernel<bf16, 2, 5, 64, false, true>(CoopArgs)",13,1,1,300.0,20.5\n')
    monkeypatch.setattr(b, "PMC_CSV", str(csvp))
    monkeypatch.setattr(b, "PMC_STAMP", str(stamp))
    stamp.write_text(json.dumps({"kernel_source_hash": b.kernel_source_hash(), "git_head": "abc1234"}))
    nbytes, note = b.pmc_traffic("lstm2_coop_bwd2_kernel", "C2")
    assert nbytes == 1500.0 * 1048576 and "abc1234" in note
    nbytes, _ = b.pmc_traffic(b.ROCPROF_NAME["lstm2_fwd_coop_g2[N=8224"], "C2")
    assert nbytes == 320.5 * 1048576
    assert b.pmc_traffic("lstm2_coop_bwd2_kernel", "C5")[0] is None                  # another workload: honest null
    assert b.pmc_traffic("no_such_kernel", "C2")[0] is None
    stamp.write_text(json.dumps({"kernel_source_hash": "0" * 16, "git_head": "abc1234"}))
    nbytes, note = b.pmc_traffic("lstm2_coop_bwd2_kernel", "C2")                      # kernels changed since the pass
    assert nbytes is None and "stale" in note


def test_algorithmic_work_matches_the_survey_figures():
    """bench.py's FLOP / byte formulas against SURVEY.md section 8(d)'s numbers for BASELINE C2 and C5"""
    b = _bench()
    assert abs(b.step_flops(32, 251, 5) / 1.968e13 - 1) < 5e-3
    assert abs(b.step_flops(8, 1876, 8) / 3.65e13 - 1) < 5e-3
    fam = b.hbm_family_bytes(32, 64000, 251, 5, 15_198_636, 2)
    assert abs(fam["stft"][0] / 57.7e6 - 1) < 0.02 and abs(fam["cirm_build_compress"][0] / 49.5e6 - 1) < 0.01
    assert abs(fam["cirm_decompress_apply"][0] / 57.8e6 - 1) < 0.01 and abs(fam["subband_staging_fwd"][0] / 66.6e6 - 1) < 0.01
    assert abs(fam["gs_and_loss"][0] / 230e6 - 1) < 0.02 and abs(fam["adam"][0] / 426e6 - 1) < 0.01


def test_summarize_pmc_on_a_synthetic_counter_file(tmp_path):
    hdr = "Correlation_Id,Dispatch_Id,Agent_Id,Queue_Id,Process_Id,Thread_Id,Grid_Size,Kernel_Id,Kernel_Name,Workgroup_Size,LDS_Block_Size,Scratch_Size,VGPR_Count,Accum_VGPR_Count,SGPR_Count,Counter_Name,Counter_Value,Start_Timestamp,End_Timestamp\n"
    row = "1,{d},0,1,1,1,64,1,\"{k}\",64,0,0,8,0,8,{c},{v},0,1\n"
    f, w = tmp_path / "f.csv", tmp_path / "w.csv"
    f.write_text(hdr + row.format(d=1, k="kern_a(int)", c="FETCH_SIZE", v=1024) + row.format(d=2, k="kern_a(int)", c="FETCH_SIZE", v=3072)
                 + row.format(d=3, k="kern_b()", c="FETCH_SIZE", v=10))
    w.write_text(hdr + row.format(d=1, k="kern_a(int)", c="WRITE_SIZE", v=512) + row.format(d=2, k="kern_a(int)", c="WRITE_SIZE", v=512))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "summarize_pmc.py"), str(f), str(w)], capture_output=True,
                         text=True, check=True).stdout.strip().splitlines()
    assert out[0].startswith("kernel,launches,")
    a = out[1].split(",")
    assert a[0] == "kern_a(int)" and a[1] == "2" and a[2] == "4096" and a[3] == "1024"
    assert float(a[4]) == 2 * 4096 / 1024 / 2 and float(a[5]) == 0.5          # MB per launch: fetch doubled (gfx950), write as is


def test_dump_outputs_stays_within_budget_and_samples_deterministically(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 .npy files, small arrays whole, an over-budget array as the same seeded sample on
    every run, complex log entries as (real, imag) pairs, the echoed inputs left out"""
    import json
    import numpy as np
    import torch
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 40_000)
    net = torch.nn.Linear(3, 2)
    big = torch.arange(20_000, dtype=torch.float32).reshape(100, 200)
    res = (torch.ones(4), torch.tensor(0.5, dtype=torch.float64),
           {"w_mat": big, "pred_crm": torch.ones(3, dtype=torch.bfloat16),
            "err_proj": torch.complex(torch.ones(4, 2), -torch.ones(4, 2)), "noisy_complex": torch.ones(8)})
    host = b.step_outputs(res, net)
    assert "noisy_complex" not in host and host["err_proj"].shape == (4, 2, 2)
    assert host["objective"].dtype == torch.float64 and host["pred_crm"].dtype == torch.float32
    assert host["direction_net_params"].numel() == 8
    runs = []
    for d in (tmp_path / "a", tmp_path / "b"):
        man = b.dump_outputs(str(d), host)
        assert sorted(p.name for p in d.iterdir()) == sorted(k + ".npy" for k in host)        # nothing but the arrays
        runs.append({p.name: np.load(p) for p in d.glob("*.npy")})
        assert sum(p.stat().st_size for p in d.glob("*.npy")) <= 40_000 + 128 * len(runs[-1])      # + the .npy headers
    json.dumps(man)                                                                      # goes into the JSON line
    assert set(runs[0]) == {k + ".npy" for k in host} and all(v.dtype in (np.float32, np.float64) for v in runs[0].values())
    assert "sampled" in man["arrays"]["w_mat"] and "sampled" not in man["arrays"]["reconst_err"]
    np.testing.assert_array_equal(runs[0]["reconst_err.npy"], np.ones(4, np.float32))
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k])
    w = runs[0]["w_mat.npy"]
    assert w.size == man["arrays"]["w_mat"]["sampled"] and np.all(np.diff(w) > 0)    # sorted flat indices of an increasing array


def test_a_plain_run_measures_nothing_beyond_its_timed_steps():
    """`bench.py --gpus 1 --steps N --warmup W` stays lean; --full adds the per-launch pass, the fp32 steps and the CPU
    baseline on one GPU, and each --no-* option still leaves its pass out there"""
    b = _bench()
    none = {"families": False, "fp32": False, "cpu_baseline": False}
    assert b.extra_passes(b.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"]), 1) == none
    assert b.extra_passes(b.parse_args(["--no-fp32"]), 1) == none
    assert b.extra_passes(b.parse_args(["--full"]), 1) == {"families": True, "fp32": True, "cpu_baseline": True}
    assert b.extra_passes(b.parse_args(["--full", "--gpus", "2"]), 2) == none
    assert b.extra_passes(b.parse_args(["--full", "--precision", "fp32"]), 1)["fp32"] is False
    assert b.extra_passes(b.parse_args(["--full", "--no-families", "--no-cpu-baseline"]), 1) == \
        {"families": False, "fp32": True, "cpu_baseline": False}


def test_config_c3_forwards_the_cpu_baseline_choice_to_the_inpainting_bench():
    """--config c3 runs tools/bench_inpainting.py, which times its CPU baseline unless told not to: only --full lets it"""
    b = _bench()

    def argv(*args):
        a = b.parse_args(["--config", "c3", *args])
        return b.inpainting_argv(a, b.extra_passes(a, 1))
    assert argv("--steps", "5", "--warmup", "2") == ["--steps", "5", "--warmup", "2", "--precision", "bf16", "--no-cpu-baseline"]
    assert "--no-cpu-baseline" not in argv("--full")
    assert "--no-cpu-baseline" in argv("--full", "--no-cpu-baseline")
    assert argv("--dump-outputs", "d")[-2:] == ["--dump-outputs", "d"]
