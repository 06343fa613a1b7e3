"""bench.py's one-line contract with the driver, checked on the GPU with a small workload: the fields the driver parses, the
`roofline` and `cpu_baseline` objects of a --full run, and the internal consistency of the line (value from its own ms_per_step,
frac from achieved / peak, traffic only for the workload the counters ran); a plain run prints the headline alone."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_carries_what_the_driver_and_the_judge_read():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "144",
                          "--full", "--no-extras", "--cpu-seconds", "2"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    for key, want in (("unit", "frame-pairs/s"), ("n_gpus", 1), ("steps", 3), ("warmup", 1), ("higher_is_better", True),
                      ("scaling", "weak"), ("vs_baseline", None), ("dtype", "f32")):
        assert line[key] == want, key
    assert line["metric"].startswith("frame-pairs/s (640x480, 4-level GN align)")
    assert "synthetic" in line["data"] and "workload" in line["config"] and "model" not in line["config"]
    # value = pairs of the timed region / its time
    assert line["value"] == pytest.approx(144 * 3 / (line["ms_per_step"] * 3e-3), rel=1e-6)
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9) and 0.02 < r["frac"] < 0.8
    assert r["launches"] > 0 and r["avg_launch_us"] > 0
    assert r["achieved"] == pytest.approx(r["alg_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9, rel=1e-6)
    assert r["traffic"] is None and r["traffic_source"] is None  # 144 pairs per step is not the workload the counters ran
    assert 0.0 <= r["speculation_waste"]["discarded_fraction_of_submitted_bytes"] < 0.2
    c = line["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["unit"] == "frame-pairs/s" and c["value"] > 0 and c["sample"]
    assert line["value"] > 50 * c["value"]  # a GPU that is not two orders above one CPU core is not running the HIP path


FULL_ONLY = ("timed_region_check", "max_deviation_from_single_match", "single_pair_latency_ms", "single_pair_latency",
             "prep_ms_per_frame", "end_to_end_ms_per_frame_one_stream", "roofline", "roofline_isolated_kernel", "cpu_baseline",
             "sensor_noise_workload", "host_rcpps_mode", "no_stats_variant", "cpu_baseline_many_threads", "tile_shard")


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_alone():
    """Without --full the run sets up, warms up, times its steps and prints the line: the driver's fields with the meaning they
    have in a --full run, and none of the side measurements."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "144"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    for key, want in (("unit", "frame-pairs/s"), ("n_gpus", 1), ("steps", 3), ("warmup", 1), ("higher_is_better", True),
                      ("scaling", "weak"), ("vs_baseline", None), ("dtype", "f32"), ("full", False)):
        assert line[key] == want, key
    assert line["metric"].startswith("frame-pairs/s (640x480, 4-level GN align)")
    assert line["config"]["pairs_per_step_per_gpu"] == 144 and line["iterations_per_pair"] > 0
    assert line["value"] == pytest.approx(144 * 3 / (line["ms_per_step"] * 3e-3), rel=1e-6)
    assert not [k for k in FULL_ONLY if k in line]


def test_full_is_off_by_default_and_the_counter_leg_implies_it(monkeypatch):
    """The counter passes summarise the launches the line's roofline section counts: a --counter-leg child runs that section."""
    B = _bench()
    for argv, full, extras in ((["--steps", "2"], False, True), (["--steps", "2", "--full"], True, True),
                               (["--steps", "1", "--counter-leg"], True, False)):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        args = B.parse()
        assert args.full is full and (not args.no_extras) is extras, argv


@pytest.mark.gpu
def test_counter_passes_select_the_timing_pass_and_measure_its_traffic():
    """roofline.traffic is a property of the run that prints it (round 5): bench.py brackets its timing pass with two k_marker
    dispatches and starts the rocprofv3 counter passes itself (dvo_slam_amd/pmc.py).  Here the same machinery on a small workload:
    the three child passes run, the summaries find exactly the k_tick dispatches bench.py timed (every form of the kernel between the
    markers), the writes are what the algorithm writes plus the unselected pixels' markers and the block records, and the calibrated
    traffic is of the size of the algorithmic bytes -- no wasted re-reads."""
    import shutil

    sys.path.insert(0, ROOT)
    from dvo_slam_amd import pmc

    if pmc.rocprofv3_path() is None or not shutil.which("python3"):
        pytest.skip("rocprofv3 is not installed on this box")
    leg = ["--counter-leg", "--steps", "1", "--warmup", "0", "--prime", "1", "--batch", "288", "--threads", "2", "--in-flight", "72"]
    live = pmc.measure_live(os.path.join(ROOT, "bench.py"), leg, timeout_s=300.0)
    t = live["traffic"]
    assert t["launches_averaged"] > 10 and t["launches_averaged"] == t["launches_of_the_write_pass"]
    assert 1.0 <= t["write_ratio_to_algorithmic"] <= 1.6, t["write_ratio_to_algorithmic"]
    lo, hi = t["wasted_traffic_ratio_bounds"]
    assert 0.3 < lo <= t["wasted_traffic_ratio_calibrated"] <= hi < 2.0, (lo, t["wasted_traffic_ratio_calibrated"], hi)
    assert t["traffic_bytes_per_launch"] == pytest.approx((2 * t["FETCH_SIZE_kb_avg_per_launch"] + t["WRITE_SIZE_kb_avg_per_launch"]) * 1024)
    i = live["issue"]
    assert "error" not in i, i
    assert i["mfma_wave_instructions"] > 0 and i["valu_wave_instructions"] > 5 * i["mfma_wave_instructions"]


def _bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _load_dump(path):
    import numpy as np

    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def _fake_step(n, seed):
    """n result structs as dvo_amd_match_wait fills them: three levels of 0..4 iterations, every field a distinct value"""
    import ctypes as C

    import numpy as np

    from dvo_slam_amd import capi

    rng = np.random.default_rng(seed)
    res, its = (capi.CResult * n)(), []
    for i in range(n):
        buf = (capi.CIterationStats * 12)()
        its.append(buf)
        r = res[i]
        r.iterations, r.iterations_capacity = C.cast(buf, C.POINTER(capi.CIterationStats)), 12
        r.transformation[:] = list(rng.standard_normal(16))
        r.information[:] = list(rng.standard_normal(36))
        r.loglik = rng.standard_normal()
        r.n_levels = 3
        for l in range(3):
            L = r.levels[l]
            L.id, L.max_valid_pixels, L.valid_pixels, L.termination = 2 - l, 1000 >> l, int(rng.integers(1, 900)), l
            L.n_iterations, L.first_iteration = int(rng.integers(0, 5)), r.n_iterations
            for k in range(L.n_iterations):
                it = buf[r.n_iterations + k]
                it.id, it.valid_constraints, it.has_increment = k, int(rng.integers(1, 900)), k % 2
                for name in ("tdist_loglik", "prior_loglik"):
                    setattr(it, name, rng.standard_normal())
                for name, size in (("tdist_mean", 2), ("tdist_precision", 4), ("increment", 6), ("information", 36),
                                   ("estimate", 16), ("initial", 16)):
                    getattr(it, name)[:] = list(rng.standard_normal(size))
            r.n_iterations += L.n_iterations
    res._keepalive = its
    return res, its


def test_dump_outputs_writes_the_last_steps_results_as_a_caller_receives_them(tmp_path):
    """bench.py --dump-outputs (no GPU needed: the writer on result structs filled here): every pair of the step in step order,
    whichever host thread collected it, each array float64, matrices and iterations exactly as capi.Result gives them; above the
    size limit a sample that is the same from run to run and stays within the limit."""
    import numpy as np

    from dvo_slam_amd import capi

    B = _bench()
    n = 60
    threads = [_fake_step(n // 2, seed) for seed in (1, 2)]
    ix = [list(range(0, n, 2)), list(range(1, n, 2))]  # dealt as sharding.split_for_threads deals a step over two threads
    kept = [(ix[t], threads[t][0]) for t in range(2)]
    want = [None] * n
    for t in range(2):
        for k, i in enumerate(ix[t]):
            want[i] = capi.Result(threads[t][0][k], threads[t][1][k])

    B.dump_outputs(str(tmp_path / "all"), kept, n)
    d = _load_dump(tmp_path / "all")
    assert all(a.dtype == np.float64 for a in d.values())
    assert np.array_equal(d["pair"], np.arange(n))
    assert np.array_equal(d["transformation"], np.stack([w.Transformation for w in want]))
    assert np.array_equal(d["information"], np.stack([w.Information for w in want]))
    assert np.array_equal(d["log_likelihood"], [w.LogLikelihood for w in want])
    assert np.array_equal(d["level_valid_pixels"], [[L["ValidPixels"] for L in w.Levels] for w in want])
    assert np.array_equal(d["level_termination"], [[L["TerminationCriterion"] for L in w.Levels] for w in want])
    off = d["iteration_offset"].astype(int)
    for p, w in enumerate(want):
        rows = [it for L in w.Levels for it in L["Iterations"]]
        assert off[p + 1] - off[p] == len(rows) == sum(d["level_n_iterations"][p])
        for j, it in enumerate(rows):
            q = off[p] + j
            assert d["iteration_valid_constraints"][q] == it["ValidConstraints"]
            assert d["iteration_tdist_loglik"][q] == it["TDistributionLogLikelihood"]
            assert np.array_equal(d["iteration_tdist_precision"][q], it["TDistributionPrecision"])
            assert np.array_equal(d["iteration_increment"][q], it["EstimateIncrement"])
            assert np.array_equal(d["iteration_information"][q], it["EstimateInformation"])
            assert np.array_equal(d["iteration_estimate"][q], it["estimate"])

    limit = 2**16 + 40_000
    B.dump_outputs(str(tmp_path / "s1"), kept, n, limit=limit)
    B.dump_outputs(str(tmp_path / "s2"), kept, n, limit=limit)
    s1, s2 = _load_dump(tmp_path / "s1"), _load_dump(tmp_path / "s2")
    assert s1.keys() == s2.keys() == d.keys() and all(np.array_equal(s1[k], s2[k]) for k in s1)
    take = s1["pair"].astype(int)
    assert 0 < len(take) < n and np.all(np.diff(take) > 0)
    assert np.array_equal(s1["transformation"], d["transformation"][take])
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= limit


def test_bench_refuses_fewer_than_one_timed_step():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps" in out.stderr


@pytest.mark.gpu
def test_dump_outputs_are_the_timed_paths_results(tmp_path):
    """bench.py --dump-outputs on the GPU: the dumped results of the last timed step are the single match() of the same pair bit for
    bit (a pair's result is a function of its inputs alone, tests/test_determinism.py), per-iteration statistics included."""
    import numpy as np

    from dvo_slam_amd import capi, synth

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "144",
                          "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(dump)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = _load_dump(dump)
    assert np.array_equal(d["pair"], np.arange(144))
    assert sum(os.path.getsize(dump / f) for f in os.listdir(dump)) <= 64 * 10**6
    B = _bench()
    W, H, levels = 640, 480, 4
    K = synth.intrinsics_for(W, H)
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    off = d["iteration_offset"].astype(int)
    for i in (0, 13, 77, 143):
        r, c = B.pair_index(i, 12, 96)
        fr, fc = B.workload_ref_frame(synth, W, H, 0, r), B.workload_cur_frame(synth, W, H, 0, c)
        want = trk.match(capi.RgbdImagePyramid(fr[0], fr[1], K, levels), capi.RgbdImagePyramid(fc[0], fc[1], K, levels))
        assert np.array_equal(d["transformation"][i], want.Transformation), i
        assert np.array_equal(d["information"][i], want.Information), i
        assert d["log_likelihood"][i] == want.LogLikelihood, i
        rows = [it for L in want.Levels for it in L["Iterations"]]
        assert off[i + 1] - off[i] == len(rows), i
        assert np.array_equal(d["iteration_tdist_loglik"][off[i]:off[i + 1]], [it["TDistributionLogLikelihood"] for it in rows]), i
        assert np.array_equal(d["iteration_estimate"][off[i]:off[i + 1]], np.stack([it["estimate"] for it in rows])), i
