"""CPU-side checks of the measurement harness: weak-scaling image sizes, the algorithmic-bytes fixture and the
committed round profile follow the bench contract."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_weak_scaling_image_sizes():
    import bench

    assert bench.image_size(1, 1920, 1080) == (1920, 1080)
    assert bench.image_size(4, 1920, 1080) == (3840, 2160)  # BASELINE config 4 resolution
    for n in (2, 8):
        w, h = bench.image_size(n, 1920, 1080)
        assert w % 8 == 0 and abs(w * h / (n * 1920 * 1080) - 1) < 0.01 and abs(w / h - 16 / 9) < 0.01


def test_algorithmic_bytes_fixture_and_formula():
    import oracle_py

    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "algbytes.json")))["atrium262k_1080p_16spp_d8"]
    assert 1000 < fx["traversal_bytes_per_ray"] < fx["bytes_per_ray"] < 6000  # SURVEY 8d expectation: 2-5 KB/ray
    c = dict(nodes_visited=10, tris_tested=3, hits=2, diffuse_hits=1, tex_taps=4, pixels=5)
    assert oracle_py.algorithmic_bytes(c) == 64 * 10 + 48 * 3 + 220 * 2 + 32 + 16 * 4 + 16 * 5
    assert oracle_py.algorithmic_bytes(c, frame_gt0=True) == oracle_py.algorithmic_bytes(c) + 16 * 5


def test_default_sizes_follow_baseline_configs():
    """N = 1 -> config 3 (1920x1080); N > 1 -> config 4 (one 3840x2160 frame, strong scaling) unless --weak."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "(3840, 2160) if world > 1 else (1920, 1080)" in src and 'scaling = "strong"' in src
    # the N > 1 line carries the single-GPU rate of the SAME frame, so that the first hardware curve is not read against the 1080p line
    assert "same_frame_single_gpu_Mrays_s" in src and "efficiency_vs_same_frame" in src


def test_product_path_of_bench_does_not_touch_the_oracle():
    """Only the cpu_baseline leg may import from oracle/ (the camera comes from the product's host library)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    head, leg = src.split("# ---- CPU oracle on a bounded sample", 1)
    assert "import oracle_py" not in head and 'os.path.join(ROOT, "oracle")' not in head and "camera_np" not in src
    assert "import oracle_py" in leg and "host_py.global_uniforms" in head


def test_bench_self_launches_its_ranks_when_no_launcher_did(tmp_path):
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment (how a driver may call the N > 1 case) must start the two
    ranks itself -- torch.distributed.run as a CHILD, before any GPU call -- and relay rank 0's single JSON line.  Rehearsed
    on the CPU with the gloo self-test mode (no GPU work): rendezvous on 127.0.0.1, one all_reduce over both ranks."""
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-selftest"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d == {"launch_selftest": True, "n_gpus": 2, "gpus_arg": 2, "rank_sum": 3.0}
    assert "torch.distributed.run" in p.stderr and "--nproc-per-node=2" in p.stderr and "127.0.0.1" in p.stderr
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "os.exec" not in src  # a process that has touched the GPU is never replaced; the launcher is a child


def test_bench_accepts_a_scene_file():
    """--gltf PATH runs a supplied scene (the reference's config.json scenes are git-ignored upstream) through the product's C++
    loader in the same harness; the GPU run of it is tests/test_host_layer.py::test_bench_runs_a_supplied_gltf."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "host_py.load_gltf(args.gltf)" in src and '"--gltf"' in src and '"--eye"' in src


def test_round3_bench_line_prices_the_binding_resource():
    import pytest

    path = os.path.join(ROOT, "profiles", "r03_bench.json")
    if not os.path.exists(path):
        pytest.skip("no round-3 bench line committed yet")
    d = json.loads(open(path).read())
    r = d["roofline"]
    assert r["bound"] == "valu-issue" and r["unit"] == "G wave-instr/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0 < r["frac_nominal"] < r["frac"] <= 1.0 and r["pmc_stale"] is False
    for sub in ("hbm_own_bytes", "contract", "l2_gather", "traffic_detail"):
        assert sub in r, sub
    assert r["contract"]["frac"] > 1.0 and "NOT a bound" in r["contract"]["note"] and "NOT a bound" in r["hbm_own_bytes"]["note"]
    assert r["traffic"] is not None and r["traffic_detail"]["over_algorithmic_bytes"] < 1.0
    cb = d["cpu_baseline"]
    assert cb["cores"] > 1 and cb["single_thread"]["cores"] == 1 and 0 < cb["single_thread"]["value"] < cb["value"] and cb["cpu_model"]


def test_round4_bench_line_says_what_follows_from_the_guide():
    """Top-level roofline.frac = achieved / the guide-derived issue peak (1228.8 G wave-instr/s); the calibrated figure is kept beside
    it; the CPU baseline ran on every thread the process may use; the Sponza-like tessellation is quoted next to the headline."""
    import pytest

    path = os.path.join(ROOT, "profiles", "r04_bench.json")
    if not os.path.exists(path):
        pytest.skip("no round-4 bench line committed yet")
    d = json.loads(open(path).read())
    r = d["roofline"]
    assert r["bound"] == "valu-issue" and abs(r["peak"] - 1228.8) < 1e-6 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["peak_calibrated"] < r["peak"] and r["frac"] < r["frac_calibrated"] <= 1.0 and r["pmc_stale"] is False
    assert r["kernel_clock_ghz"] is None or 1.0 < r["kernel_clock_ghz"] < 3.0
    assert d["scaling"] == "strong" and d["n_gpus"] == 1
    cb = d["cpu_baseline"]
    assert cb["cores"] == cb["cpus_available_to_this_process"] and cb["single_thread"]["cores"] == 1
    assert cb["cores"] <= 16 or cb["threads_16"]["cores"] == 16
    cfg = d["config"]
    assert cfg["frames_per_call"] >= 1 and cfg["frames_in_flight"] >= 1
    nu = cfg["nonuniform_variant"]
    assert 0.5 < nu["ratio_to_headline"] < 1.2 and abs(nu["ratio_to_headline"] - nu["Mrays_s"] / d["value"]) < 1e-9


def test_round2_bench_line_roofline_is_a_fraction():
    import pytest

    path = os.path.join(ROOT, "profiles", "r02_bench.json")
    if not os.path.exists(path):
        pytest.skip("no round-2 bench line committed yet")
    d = json.loads(open(path).read())
    r = d["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["issue"]["peak"] > 0 and (r["issue"]["frac"] is None or 0 < r["issue"]["frac"] <= 1.0)
    assert "contract" in r and "builds" in d["config"] and d["config"]["source_hash"]


def test_committed_bench_line_follows_contract():
    path = os.path.join(ROOT, "profiles", "r01_bench.json")
    if not os.path.exists(path):
        import pytest

        pytest.skip("no committed bench line yet")
    d = json.loads(open(path).read())
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "Mrays/s" and d["vs_baseline"] is None and d["dtype"] == "f32" and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1


def test_issue_mix_estimate_is_the_ceiling_a_share_of_half_rate_opcodes_allows():
    import bench

    """roofline.issue_mix (bench.issue_mix_block): h = share of half-rate instructions, ceiling = 1 / (1 + h) of the full-rate peak."""
    mix = {"node_test": {"valu": 200, "half_rate": 100}, "loop_rest": {"valu": 100, "half_rate": 0}}
    b = bench.issue_mix_block(mix, valu_per_ray=100.0, node_wave_steps_per_ray=16.0 / 64.0, frac_of_peak=0.5)
    assert b["valu_instr_per_wave"] == 6400.0 and b["node_test_instr_per_wave"] == 3200.0
    assert abs(b["half_rate_share"] - 0.25) < 1e-12 and abs(b["ceiling_frac_of_peak"] - 0.8) < 1e-12
    assert abs(b["frac_of_mix_ceiling"] - 0.625) < 1e-12
    # the committed static mix (tools/isa_blocks.py --json) has the shape the estimate reads; bench.py ignores it when its source hash is stale
    m = json.load(open(os.path.join(ROOT, "profiles", "isa_mix.json")))
    assert m["node_test"]["valu"] >= m["node_test"]["half_rate"] > 0 and m["loop_rest"]["valu"] > 0 and "source_hash" in m
    r = json.load(open(os.path.join(ROOT, "profiles", "r04_bench.json")))["roofline"]
    steps = r["per_ray"]["nodes_visited"] / (64.0 * r["per_ray"]["node_step_lane_efficiency"])
    e = bench.issue_mix_block(m, r["valu_wave_instr_per_ray"], steps, r["frac"])
    assert 0.6 < e["ceiling_frac_of_peak"] < 0.8 and r["frac"] < e["frac_of_mix_ceiling"] < 1.0


def test_cpu_baseline_threads_deal_chunks_and_agree_with_one_thread():
    """cpu_baseline (round 5): the oracle deals 32-pixel chunks of the sampled rows to its threads dynamically and every thread counts
    into a block of its own (VERDICT r04 'weak' 6: whole rows per thread and false-shared counters made 256 threads slower than 16).
    Pixels and counters must not depend on the thread count, ragged last chunk included; bench.py sizes the sample to at least eight
    chunks per thread and uses the cgroup's CPU quota when it is below the affinity mask."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import camera_np
    import oracle_py
    from vkrt_amd.flat_scene import FlatScene, make_push_constants, uniforms_from_matrices

    flat = FlatScene.load_npz(os.path.join(ROOT, "tests", "golden", "cornell_flat.npz"))
    W, H = 75, 40  # 75 = two whole chunks + a ragged one of 11 pixels
    cam = uniforms_from_matrices(*camera_np.global_uniforms(width=W, height=H))
    pc = make_push_constants(samples=2, depth=3, frame=0, lights_count=len(flat.lights))
    orc = oracle_py.OracleScene(flat)
    rows = np.array([0, 7, 8, 21, 39], np.uint32)
    ref, c1 = orc.render(pc, cam, W, H, seed=3, rows=rows, threads=1)
    for nt in (3, 16, 61):
        img, c = orc.render(pc, cam, W, H, seed=3, rows=rows, threads=nt)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)) and c == c1, nt
    assert c1["pixels"] == len(rows) * W and c1["rays_closest"] > 0
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "min_rows = -(-8 * nthreads" in src and "cpu_quota()" in src and '"cgroup_cpu_quota": quota' in src
    osrc = open(os.path.join(ROOT, "oracle", "oracle.cpp")).read()
    assert "std::vector<Counters> cs(nt);" in osrc and "Counters c;\n    for(;;)" in osrc  # thread-local block, handed over once


def test_cpu_quota_reads_cgroup_files(tmp_path, monkeypatch):
    import builtins

    import bench

    real_open = builtins.open

    def fake(files):
        def _open(path, *a, **k):
            if isinstance(path, str) and path.startswith("/sys/fs/cgroup/"):
                if path in files:
                    f = tmp_path / path.replace("/", "_")
                    f.write_text(files[path])
                    return real_open(f, *a, **k)
                raise FileNotFoundError(path)
            return real_open(path, *a, **k)
        return _open

    monkeypatch.setattr(builtins, "open", fake({"/sys/fs/cgroup/cpu.max": "1600000 100000\n"}))
    assert bench.cpu_quota() == 16
    monkeypatch.setattr(builtins, "open", fake({"/sys/fs/cgroup/cpu.max": "max 100000\n"}))
    assert bench.cpu_quota() is None
    monkeypatch.setattr(builtins, "open", fake({"/sys/fs/cgroup/cpu/cpu.cfs_quota_us": "250000\n", "/sys/fs/cgroup/cpu/cpu.cfs_period_us": "100000\n"}))
    assert bench.cpu_quota() == 3
    monkeypatch.setattr(builtins, "open", fake({}))
    assert bench.cpu_quota() is None


def test_round5_bench_line_carries_the_shade_and_frame_rooflines():
    """profiles/r05_bench.json: roofline.shade prices k_wf_shade against the HBM peak with the fabric-side
    bytes of the committed --pmc passes (raw and x2 on the read side) and with the record bytes its stream counters give;
    roofline.frame_hbm is the whole frame's achieved HBM GB/s; cpu_baseline names the CPUs it really used."""
    path = os.path.join(ROOT, "profiles", "r05_bench.json")
    d = json.loads(open(path).read())
    assert d["metric"] == "Mrays/s" and d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["dtype"] == "f32"
    assert abs(d["value"] - d["config"]["rays_per_step"] / d["ms_per_step"] / 1e3) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "valu-issue" and r["pmc_stale"] is False and 0.4 < r["frac"] < 0.8 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert 0.6 < r["issue_mix"]["ceiling_frac_of_peak"] < 0.8 and r["frac"] < r["issue_mix"]["ceiling_frac_of_peak"]
    s = r["shade"]
    assert s["kernel"] == "k_wf_shade" and s["bound"] == "hbm" and s["peak"] == 8000.0 and s["pmc_stale"] is False
    assert abs(s["frac"] - s["achieved"] / s["peak"]) < 1e-9 and s["frac"] < s["frac_reads_x2"] < 1.0
    assert abs(s["traffic"] - (s["read_bytes_per_launch_raw"] + s["write_bytes_per_launch"])) < 1.0
    # what the kernel writes is its records: WRITE_SIZE of the counter pass and the record bytes from the stream counters agree
    assert abs(s["write_bytes_per_launch"] / s["record_bytes_out_per_launch"] - 1.0) < 0.05
    assert 80 < s["record_bytes_in_per_launch"] / s["records_per_launch"] < 112 and 0.05 < s["kernel_ms"] < 0.2
    f = r["frame_hbm"]
    assert f["unit"] == "GB/s" and abs(f["achieved"] - f["bytes_per_frame_raw"] / (d["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * f["achieved"]
    assert f["frac"] < f["frac_reads_x2"] < 1.0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == min(c["cpus_available_to_this_process"], c["cgroup_cpu_quota"] or c["cpus_available_to_this_process"])
    assert abs(c["cpu_seconds_per_wall_second"] - c["cores"]) < 0.15 * c["cores"]  # the sample kept the CPUs it claims busy
    assert c["value"] > 8 * c["single_thread"]["value"]
    # the counter summaries the line quotes belong to the same sources
    for name in ("pmc_issue.json", "pmc_traffic.json", "isa_mix.json"):
        assert json.load(open(os.path.join(ROOT, "profiles", name)))["source_hash"] == d["config"]["source_hash"], name


def test_dump_outputs_keeps_the_budget_and_a_fixed_sample(tmp_path):
    """--dump-outputs: an image that fits is written whole in float32; a larger one (the 4K frame of N > 1) keeps the same
    seeded rows on every run, their indices beside it, and all files together stay within the 64 MB budget."""
    import numpy as np
    import torch

    import bench

    small = torch.arange(6 * 5 * 4, dtype=torch.float32).reshape(6, 5, 4)
    assert bench.dump_outputs(str(tmp_path / "s"), {"image": small}) == {"image.npy": [6, 5, 4]}
    got = np.load(tmp_path / "s" / "image.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())

    big = torch.rand((2160, 3840, 4), generator=torch.Generator().manual_seed(3))
    runs = []
    for d in ("a", "b"):
        w = bench.dump_outputs(str(tmp_path / d), {"image": big})
        assert set(w) == {"image.npy", "image_rows.npy"} and w["image.npy"][1:] == [3840, 4]
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= bench.DUMP_BUDGET_BYTES
        img, rows = np.load(tmp_path / d / "image.npy"), np.load(tmp_path / d / "image_rows.npy")
        assert img.dtype == np.float32 and rows.dtype == np.float64 and len(rows) == img.shape[0] > 1000
        assert np.all(np.diff(rows) > 0) and np.array_equal(img, big.numpy()[rows.astype(np.int64)])
        runs.append(rows)
    assert np.array_equal(runs[0], runs[1])


def test_bench_refuses_zero_steps():
    import subprocess

    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr
