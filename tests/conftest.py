import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "faster-qwen3-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")

# bf16 arithmetic of the CPU oracle depends on the code path the host CPU selects (AMX, AVX-512 or AVX2 kernels in oneDNN, MKL and
# ATen; vendor-specific MKL branches; the thread count): near-tie ids differ between hosts.  Tests that pin bf16 oracle ids run
# in a child process on these paths, which every x86-64 host with AVX2 executes identically.
PINNED_CPU_NUMERICS = {"ONEDNN_MAX_CPU_ISA": "AVX2", "MKL_CBWR": "COMPATIBLE", "ATEN_CPU_CAPABILITY": "avx2",
                       "OMP_NUM_THREADS": "8", "MKL_NUM_THREADS": "8"}


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu via gpurun)")


def pytest_collection_modifyitems(config, items):
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


@pytest.fixture(scope="session")
def run_pinned_cpu():
    """run(code) -> the JSON value the child's last stdout line holds; `code` runs with the repository on sys.path under
    PINNED_CPU_NUMERICS (they take effect only before torch loads its math libraries, hence the child)."""
    def run(code, timeout=900):
        head = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'faster-qwen3-tts_amd')!r}]\n"
        r = subprocess.run([sys.executable, "-c", head + code], cwd=ROOT, env=dict(os.environ, **PINNED_CPU_NUMERICS),
                           capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    return run
