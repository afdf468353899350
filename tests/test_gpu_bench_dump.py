"""bench.py on the HIP path, as later measurements call it: a plain run (no --full) prints the
headline line only, and --dump-outputs writes the last timed step's outputs for a comparison of
two builds.  One small run (512 molecules, 2 timed steps) shared by the checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--total-mols", "512", "--mols-per-step", "256",
                        "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f.name[:-4]: np.load(f) for f in sorted(d.iterdir())}, r.stderr


def test_plain_run_reports_the_headline_only(plain_run):
    line, _, err = plain_run
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "molecules/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["metric"].startswith("molecules/sec")
    assert line["ms_per_step"] > 0
    # value = molecules of the timed steps / their time: 2 steps of 256 molecules
    assert line["value"] == pytest.approx(2 * 256 / (2 * line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None
    for k in ("inference", "view_only", "kernel_ms_per_step", "roofline_gemm"):
        assert k not in line, k
    assert "ms/step" not in err  # no per-kernel breakdown


def test_dump_holds_the_last_steps_outputs(plain_run):
    _, a, _ = plain_run
    assert a["logits"].shape == (256, 11) and a["graph_embedding"].shape == (256, 384)
    assert a["loss"].shape == (1,) and 0.0 < float(a["loss"][0]) < 10.0
    params = {n for n in a if n.startswith("param.")}
    grads = {n for n in a if n.startswith("grad.")}
    assert set(a) == {"logits", "loss", "graph_embedding"} | params | grads
    assert any(n.startswith("param.gnn.") for n in params) and any(n.startswith("param.fusion.") for n in params)
    # every gradient belongs to a parameter; only the never-used LayerNorm has none
    assert {"param." + n[5:] for n in grads} <= params
    assert {n[6:] for n in params} - {n[5:] for n in grads} == {"fusion.norm_layer.weight", "fusion.norm_layer.bias"}
    for n, v in a.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), n
        assert v.size <= 4 << 20, n
    assert any(np.abs(a[n]).max() > 0 for n in grads)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
