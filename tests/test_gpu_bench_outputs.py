"""bench.py's plain run on the GPU, in process and tiny: the headline alone, --steps timed
steps, and --dump-outputs writing the Kxx entries of the last timed step.

The dumped entries are checked against the CPU oracle on the same seeded images at the
float64 tolerance of tests/test_gpu_parity.py for the default (closed-form ReLU) numerics,
1e-8 relative, and two runs with the same arguments must dump identical bytes."""
import importlib
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from oracle import nngp_oracle as O
from oracle import specs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = "mnist_paper_convnet_gp"
N, TILE = 72, 32            # three block rows, the last one ragged (8): 6 upper tiles


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_times_steps_and_dumps_the_last_step(tmp_path, capsys):
    b = _bench()
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--config", CFG,
            "--n", str(N), "--tile", str(TILE)]
    lines, dumps = [], []
    try:
        for name in ("a", "b"):
            d = str(tmp_path / name)
            assert b.main(argv + ["--dump-outputs", d]) == 0
            out = capsys.readouterr().out.strip().splitlines()
            assert len(out) == 1                   # one JSON line, nothing else on stdout
            lines.append(json.loads(out[0]))
            assert sorted(os.listdir(d)) == ["kxx_diag.npy", "kxx_upper.npy"]
            dumps.append({k: np.load(os.path.join(d, k + ".npy"))
                          for k in ("kxx_diag", "kxx_upper")})
    finally:
        # bench.py moved the shared config module's model to the GPU in place
        importlib.import_module(f"configs.{CFG}").initial_model.to("cpu", torch.float32)
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["ms_per_step"] > 0
    pairs = N * (N - 1) // 2                       # i < j on diagonal tiles
    assert line["config"]["pairs_per_step"] == pairs
    assert line["value"] == pytest.approx(pairs / (line["ms_per_step"] * 1e-3), rel=0.02)
    # the headline alone: no other leg ran, no full-result file was named
    for leg in ("conv_stencil_roofline", "mnist_as_tf", "solve", "cifar10", "dropin", "f32",
                "fullscale", "fullscale_f32", "fullscale_cifar10", "full_result", "error"):
        assert leg not in line, leg
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert line["outputs"]["arrays"] == {"kxx_diag": [N], "kxx_upper": [N * (N + 1) // 2]}

    for k in ("kxx_diag", "kxx_upper"):
        assert dumps[0][k].dtype == np.float64
        assert dumps[0][k].tobytes() == dumps[1][k].tobytes()

    g = torch.Generator(device="cpu").manual_seed(0)
    X = torch.rand((N, 1, 28, 28), generator=g, dtype=torch.float64).numpy()
    ref = O.kernel(specs.CONFIGS[CFG](), X)
    iu = np.triu_indices(N)
    for got, want in ((dumps[0]["kxx_upper"], ref[iu]), (dumps[0]["kxx_diag"], np.diag(ref))):
        err = float(np.max(np.abs(got - want) / np.abs(want)))
        print(f"dumped entries vs oracle: worst rel err {err:.2e}")
        assert err < 1e-8
