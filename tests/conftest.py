import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "cqa-crct_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


# ---- the 2-rank data-parallel GPU test needs two FRESH processes on the GPU.  They are started here, at session start,
# before this pytest process has initialised the GPU (a process that has must not exec another program on the GPU pool);
# they run beside the other GPU tests and tests/test_ddp_gpu.py collects their results.  ONE sequencer process
# (tests/ddp_worker.py --cases) runs the cases one after another: with this process and the two ranks a GPU test may start
# itself (test_bench_contract.py), at most five processes hold the GPU at any time.
_DDP = {"workers": None}
DDP_CASE_LIMIT_S = 300.0           # per case (both ranks); a rank still running then is ended, and no later case starts


def pytest_collection_finish(session):
    """Runs after collection and before any test (so before this process touches the GPU).  The workers are only started
    when tests/test_ddp_gpu.py is among the selected items: a ``-k`` subset without it runs with the GPU to itself."""
    if os.environ.get("CRCT_NO_DDP_WORKERS") or _DDP["workers"]:
        return
    if not any(os.path.basename(str(it.fspath)) == "test_ddp_gpu.py" for it in session.items):
        return
    try:
        import torch
        n_gpus = torch.cuda.device_count()
        if n_gpus < 1:
            return
    except Exception:
        return
    import subprocess
    import tempfile
    outdir = tempfile.mkdtemp(prefix="crct_ddp_")
    cases = ("tiny", "full") + (("tiny_rccl", "full_rccl") if n_gpus >= 2 else ())      # RCCL between two processes needs two GPUs
    argv = [sys.executable, os.path.join(ROOT, "tests", "ddp_worker.py"), "--cases", outdir, str(DDP_CASE_LIMIT_S)] + list(cases)
    with open(os.path.join(outdir, "sequencer.log"), "w") as log:
        proc = subprocess.Popen(argv, stdout=log, stderr=subprocess.STDOUT)
    _DDP["workers"] = dict(outdir=outdir, cases=cases, limit_s=DDP_CASE_LIMIT_S, proc=proc)


def pytest_sessionfinish(session, exitstatus):
    w = _DDP["workers"]
    if w and w["proc"].poll() is None:
        w["proc"].terminate()                      # the sequencer ends the ranks it has running, then itself
        try:
            w["proc"].wait(timeout=30)
        except Exception:
            w["proc"].kill()
            w["proc"].wait()


@pytest.fixture(scope="session")
def ddp_workers():
    return _DDP["workers"]
