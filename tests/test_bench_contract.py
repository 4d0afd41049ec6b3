"""The committed bench line (profiles/r4_bench_n1.json, what `python bench.py --full` prints on an MI355X) keeps the
contract the driver parses: metric / unit of BASELINE.json, whole-job value, and the `roofline` and `cpu_baseline`
objects of a --full run.  Runs on CPU: it checks the artifact, not the GPU.  Below it: the command line (plain run
against --full), the self-launch path and the --dump-outputs writer on CPU, and the benchmark itself on the GPU."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = os.path.join(ROOT, "profiles", "r4_bench_n1.json")
for _old in ("r2_bench_n1.json", "r1_bench_n1.json"):
    if not os.path.exists(LINE):
        LINE = os.path.join(ROOT, "profiles", _old)


@pytest.fixture(scope="module")
def line():
    if not os.path.exists(LINE):
        pytest.skip("no committed bench line")
    with open(LINE) as f:
        rows = [r for r in f.read().strip().split("\n") if r.startswith("{")]
    assert len(rows) == 1, "bench.py prints ONE JSON line"
    return json.loads(rows[0])


def test_top_level_fields(line):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    assert base["metric"].startswith(line["metric"])          # BASELINE.json appends the configuration to the metric name
    assert line["unit"] == "QA-pairs/s" and line["higher_is_better"] is True and line["scaling"] == "weak"
    assert line["vs_baseline"] is None                           # BASELINE.md holds no published number for this metric
    assert line["data"] == "synthetic" and line["dtype"] == "bf16"
    assert "workload" in line["config"] and "model" not in line["config"]
    # value = QA pairs of all ranks / max-over-ranks step time
    per_step = line["config"]["global_batch"]
    assert abs(line["value"] - per_step / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]


def test_roofline_object(line):
    r = line["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert r["peak"] == 2500.0 and 0.0 < r["frac"] < 1.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    # achieved = algorithmic FLOPs per launch / measured launch duration
    assert abs(r["achieved"] - r["gflop_per_launch"] / r["us_per_launch"] * 1e3) / r["achieved"] < 1e-6    # GFLOP / us = PFLOP/s
    if "ffn" in r:         # round 3: the kernel group is the FFN GEMMs by model site
        assert "FFN" in r["kernel"] and r["ffn"]["fwd_dgrad"]["frac"] == r["frac"]
        for site in ("t.ffn_up.fwd", "t.ffn_down.fwd", "t.ffn_up.dgrad", "t.ffn_down.dgrad", "v.ffn_up.fwd", "v.ffn_down.fwd"):
            assert 0.0 < r["ffn"][site]["frac"] < 1.0 and r["ffn"][site]["us"] > 0


def test_cpu_baseline_object(line):
    c = line["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["unit"] == line["unit"]
    assert c["value"] > 0 and c["cores"] >= 1 and isinstance(c["sample"], str) and c["sample"]


def test_driver_entry_points_are_there():
    """__graft_entry__.py: build() (compile every HIP source for gfx950, load the library, check the ABI) and smoke() exist and
    build() works here without a GPU.  (The file was once committed EMPTY for most of a round: nothing imported it.)"""
    import importlib
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    g = importlib.import_module("__graft_entry__")
    assert callable(getattr(g, "build", None)) and callable(getattr(g, "smoke", None))
    g.build()
    for top in ("bench.py", "DESIGN.md", "INTEGRATION.md", "include/crct_hip.h", "oracle/crct_oracle.py"):
        assert os.path.getsize(os.path.join(ROOT, top)) > 1000, top


def test_full_is_an_option_that_is_off_by_default(monkeypatch):
    """`bench.py --gpus 1 --steps N --warmup W` is the plain run (set-up, warm-up, timed steps, the line); --full asks for every
    further leg, and the switches of the single legs keep their defaults, so that --full alone runs them all."""
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    plain = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
    monkeypatch.setattr(sys, "argv", plain)
    a = bench.parse()
    assert a.full is False and (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.sustained_s > 0 and a.profile_steps > 0 and not a.no_h2d_leg and not a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", plain + ["--full"])
    b = bench.parse()
    assert b.full is True
    assert {k: v for k, v in vars(b).items() if k != "full"} == {k: v for k, v in vars(a).items() if k != "full"}


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus N` with no launcher around it (the shape of the driver's 1-GPU command) starts N fresh rank
    processes itself -- the reference's mp.spawn (CRCT/train.py:356-363) -- relays rank 0's ONE JSON line, and exits with the
    first failing rank's code.  --launch-check stops every rank before it touches a GPU, so this runs on the CPU box."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR") and not k.startswith("CRCT_")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--launch-check"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [r for r in res.stdout.strip().split("\n") if r.startswith("{")]
    assert len(rows) == 1 and res.stdout.strip() == rows[0], res.stdout          # stdout carries rank 0's line and nothing else
    info = json.loads(rows[0])
    assert info["rank"] == 0 and info["world"] == 4 and info["master"].startswith("127.0.0.1:") and info["ipc_legacy"] == "0"
    for r in (1, 2, 3):                                                          # the other ranks report on stderr: each its own rank / device
        assert "rank %d: {'rank': %d, 'local_rank': %d, 'world': 4" % (r, r, r) in res.stderr
    # a rank that dies takes the job down with its exit code (its peers would wait in a collective for ever otherwise)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--launch-check"], cwd=ROOT,
                         env=dict(env, CRCT_LAUNCH_CHECK_FAIL_RANK="2"), capture_output=True, text=True, timeout=300)
    assert res.returncode == 7
    assert "rank 2 (exit 7)" in res.stderr                                      # ... and the launcher says which rank it was
    # a rank that never comes back (a peer stuck in the RCCL bootstrap): after --rank-timeout-s the launcher ends every rank it started
    # and exits 124 with each rank's last stderr lines
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check", "--rank-timeout-s", "3"], cwd=ROOT,
                         env=dict(env, CRCT_LAUNCH_CHECK_HANG_RANK="1"), capture_output=True, text=True, timeout=120)
    assert res.returncode == 124, (res.returncode, res.stderr[-1500:])
    assert "--rank-timeout-s 3" in res.stderr and "waiting for a peer that never comes" in res.stderr
    # under a launcher that has set the rendezvous already (torch.distributed.run) no further processes are started
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], cwd=ROOT,
                         env=dict(env, RANK="1", LOCAL_RANK="1", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="1"),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("rank 1:") and res.stderr.count("rank") == 0
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-check"], cwd=ROOT,
                         env=dict(env, RANK="1", WORLD_SIZE="4"), capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "does not match WORLD_SIZE" in res.stderr


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path):
    """bench.py --dump-outputs (the writer, on CPU tensors): every return value of the step as <name>.npy, nested lists flattened,
    floating data as float32, integers as float64, an output above DUMP_SAMPLE elements as the same seeded sample in every run,
    all of it under the 64 MB limit."""
    import sys
    import numpy as np
    import torch
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench

    class Core:
        flat_params = torch.arange(bench.DUMP_SAMPLE + 1000, dtype=torch.float32)
    logits = torch.randn(4, 2, dtype=torch.bfloat16)
    outputs = (torch.tensor(1.5), torch.zeros(1, 1), torch.tensor([0.25]), None, logits,
               [torch.randn(4, 1), torch.tensor(0.5), torch.ones(4, dtype=torch.int64), (torch.tensor(3), torch.tensor(2)), None], torch.zeros(1))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outputs, Core())
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(n + ".npy" for n in ("loss", "lm_loss", "nsp_loss", "nsp_scores", "regression_0", "regression_1", "regression_2",
                                                 "regression_3_0", "regression_3_1", "legend_loss", "params_after_step")), names
    total = 0
    for n in names:
        a, b = np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
    assert np.load(str(tmp_path / "a" / "loss.npy")) == np.float32(1.5)
    assert np.array_equal(np.load(str(tmp_path / "a" / "nsp_scores.npy")), logits.float().numpy())
    assert np.load(str(tmp_path / "a" / "regression_2.npy")).dtype == np.float64
    p = np.load(str(tmp_path / "a" / "params_after_step.npy"))
    assert p.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(p) >= 0) and len(np.unique(p)) > bench.DUMP_SAMPLE // 2


@pytest.mark.gpu
def test_two_rank_bench_runs_end_to_end(tmp_path):
    """The N > 1 path of bench.py as the driver launches it (`python -m torch.distributed.run --nproc-per-node 2 bench.py
    --gpus 2 ...`), on this one-GPU box with both ranks on cuda:0 and gloo between them (CRCT_BENCH_SHARE_GPU: a developer
    switch that changes the process group only): FlatGradDDP in event mode, the stats all-reduce inside the step, the
    overlapped optimizer, max-over-ranks timing, ONE JSON line from rank 0.  (Round 2 shipped for a while with an in-place
    all-reduce on the buffer the loss is a view of -- every N > 1 run died in backward; this test is the guard.)
    The self-launched run is a --full one (with the legs `common` switches off): the sustained leg and the stand-alone all-reduce
    run with the exchange on; the other three are plain runs and report neither."""
    import subprocess
    import sys
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("CRCT_")},        # bench.py refuses stray CRCT_* switches
               CRCT_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    import socket
    with socket.socket() as sock:                       # a free rendezvous port
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    common = ["--steps", "3", "--warmup", "1", "--batch", "16", "--no-cpu-baseline", "--profile-steps", "0", "--no-h2d-leg", "--no-dropout"]
    losses = {}
    for dtype in ("fp32", "bf16", "bf16+fp8"):            # the last one: BASELINE configs[4] under the exchange (bf16 payload)
        extra = ["--dtype", "fp8"] if dtype.endswith("fp8") else []
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--grad-dtype", dtype.split("+")[0]] + extra + common
        if dtype == "bf16":      # the default payload WITHOUT a launcher: exactly `python bench.py --gpus 2 ...`, which starts its own two ranks
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--grad-dtype", "bf16", "--full"] + common
        res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        rows = [r for r in res.stdout.strip().split("\n") if r.startswith("{")]
        assert len(rows) == 1, rows
        line = json.loads(rows[0])
        assert line["n_gpus"] == 2 and line["steps"] == 3 and line["scaling"] == "weak"
        assert line["config"]["global_batch"] == 2 * 16 and line["value"] > 0
        pay = line["config"]["gradient_allreduce"]["step_payload"]
        assert pay["dtype"] == dtype.split("+")[0] and pay["collectives_issued_inside_the_backward_call"] == pay["buckets"] >= 8
        if dtype.startswith("bf16"):      # the weight-gradient GEMMs wrote the communication buffer themselves (lazy clears from step 2 on)
            assert pay["weight_gradients_written_as_bf16_by_the_gemms"] is True
        assert line["dtype"] == ("fp8" if dtype.endswith("fp8") else "bf16")
        comm = line["config"]["gradient_allreduce"]
        if dtype == "bf16":      # --full: 2 s worth of steps (at the timed steps' pace) after the timed ones, and the flat gradient buffer all-reduced on its own
            assert line["config"]["sustained"]["steps"] >= 2.0 / (line["ms_per_step"] * 1e-3) and line["config"]["sustained"]["seconds"] > 0
            assert comm["allreduce_ms"] > 0 and comm["bus_GBps"] > 0
        else:
            assert line["config"]["sustained"] is None and comm["allreduce_ms"] is None and comm["bus_GBps"] is None
        assert comm["allreduce_bytes"] > 0 and comm["rccl"]["world"] == 2
        losses[dtype] = line["config"]["global_loss"]
    # the same four optimizer steps by ONE rank on the concatenation of the two ranks' batches: the data-parallel run must land on
    # the same mean loss (1/world folded into the gradient seeds, SUM all-reduce, every rank applying the same update)
    env1 = {k: v for k, v in env.items() if k != "CRCT_BENCH_SHARE_GPU"}
    dump = str(tmp_path / "outputs")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--emulate-ranks", "2", "--dump-outputs", dump] + common,
                         cwd=ROOT, env=env1, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    one = json.loads([r for r in res.stdout.strip().split("\n") if r.startswith("{")][0])
    assert one["config"]["global_batch"] == 32
    # --dump-outputs: the loss of the LAST timed step is the one the line reports
    import numpy as np
    assert float(np.load(os.path.join(dump, "loss.npy"))) == one["config"]["final_loss"]
    assert np.load(os.path.join(dump, "nsp_scores.npy")).shape[0] == 32
    assert np.isfinite(np.load(os.path.join(dump, "params_after_step.npy"))).all()
    ref = one["config"]["global_loss"]
    assert abs(losses["fp32"] - ref) <= 2e-3 * abs(ref), (losses, ref)       # different batch split -> other summation orders / bf16 roundings
    assert abs(losses["bf16"] - ref) <= 5e-3 * abs(ref), (losses, ref)
    assert abs(losses["bf16+fp8"] - ref) <= 3e-2 * abs(ref), (losses, ref)   # e4m3 / e5m2 GEMMs: the loss moves by a per cent or so


LEGS = ("sustained", "h2d_inclusive", "critical_path")      # config keys of legs with steps of their own: null in a plain line


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_adds_every_leg(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` reports the headline and what describes the timed steps, and none of the
    legs that take steps of their own; --full reports them all (the CPU leg switched off here: it alone takes ~20 s) next to the
    same headline fields.  Without dropout both runs compute the same steps, so the last timed step's loss is the same number and
    the arrays of --dump-outputs are the same bits: --full adds work after the timed steps and changes nothing in them."""
    import subprocess
    import sys
    import numpy as np
    env = {k: v for k, v in os.environ.items() if not k.startswith("CRCT_") and k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    lines = {}
    for kind, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--sustained-s", "0.2"])):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16", "--no-dropout",
               "--dump-outputs", str(tmp_path / kind)] + extra
        res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        rows = [r for r in res.stdout.strip().split("\n") if r.startswith("{")]
        assert len(rows) == 1, rows
        lines[kind] = json.loads(rows[0])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["metric"] == "QA-pairs/sec training step (whole node)" and line["unit"] == "QA-pairs/s" and line["higher_is_better"] is True
        assert line["dtype"] == "bf16" and line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1
        assert line["ms_per_step"] > 0 and abs(line["value"] - 16 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
        assert line["config"]["schedule"]["optimizer_overlap"] is True and line["config"]["host_enqueue_ms_per_step"] > 0
    # the plain line: the same config keys, nothing measured outside the timed steps
    assert set(plain["config"]) == set(full["config"])
    for key in ("roofline", "cpu_baseline", "value_h2d_inclusive", "ms_per_step_h2d_inclusive"):
        assert key not in plain, key
    assert all(plain["config"][k] is None for k in LEGS) and plain["config"]["gemm_sites"] == [] and plain["config"]["gemm_variants"] == []
    # the --full line: every leg that was asked for
    assert "cpu_baseline" not in full                                        # --no-cpu-baseline
    assert full["config"]["sustained"]["steps"] >= 0.2 / (full["ms_per_step"] * 1e-3) and full["config"]["sustained"]["ms_per_step"] > 0      # 0.2 s at the timed pace
    assert full["value_h2d_inclusive"] == full["config"]["h2d_inclusive"]["qa_pairs_per_s"] > 0
    assert full["config"]["critical_path"]["launches_per_step"] > 100 and len(full["config"]["gemm_sites"]) > 20 and full["config"]["gemm_variants"]
    r = full["roofline"]
    assert r["bound"] == "mfma" and abs(r["peak"] - 2500.0) < 1e-6 and 0.0 < r["frac"] < 1.0 and r["ffn"]["t.ffn_up.fwd"]["us"] > 0      # peak = FLOPs / ideal time: a quotient
    # the timed steps are the same steps
    assert plain["config"]["final_loss"] == full["config"]["final_loss"]
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(os.listdir(str(tmp_path / "full"))) and "params_after_step.npy" in names
    for n in names:
        assert np.array_equal(np.load(str(tmp_path / "plain" / n)), np.load(str(tmp_path / "full" / n))), n
