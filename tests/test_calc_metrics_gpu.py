"""The calc_metrics tool on the device: the CLI builds the package's generator from the run's config and a snapshot, runs FID and
precision / recall with --device=cuda, and the launch log shows the fused k-NN kernels."""
import json

import numpy as np
import pytest

import knn_manifold_util as ku
from test_calc_metrics_cpu import _detectors, _run
from style_big_gan_amd import calc_metrics
from style_big_gan_amd.metrics import scores

pytestmark = pytest.mark.gpu


def test_cli_run_on_the_device(dev, tmp_path, capsys, monkeypatch):
    _, overrides, snap, _ = _run(tmp_path, n_images=24)
    det = _detectors(str(tmp_path / "det"))
    fid, pr = scores.compute_fid, scores.compute_pr
    monkeypatch.setattr(scores, "compute_fid", lambda opts, max_real, num_gen, **kw: fid(opts, max_real=max_real, num_gen=24, **kw))
    monkeypatch.setattr(scores, "compute_pr", lambda opts, max_real, num_gen, nhood_size, row_batch_size, col_batch_size, **kw:
                        pr(opts, max_real=max_real, num_gen=32, nhood_size=nhood_size, row_batch_size=16, col_batch_size=16, **kw))
    argv = overrides + [f"--snapshot={snap}", f"--detector={det}", "--metrics=fid50k_full,pr50k3_full", "--device=cuda", "--verbose=0"]
    capsys.readouterr()
    with ku.pr_launches() as seen:
        results = calc_metrics.run_calc_metrics(argv)
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert [line["metric"] for line in lines] == ["fid50k_full", "pr50k3_full"]
    assert np.isfinite(lines[0]["results"]["fid50k_full"]) and lines[0]["results"]["fid50k_full"] == results["fid50k_full"].results.fid50k_full
    assert all(0 <= lines[1]["results"][key] <= 1 for key in ("pr50k3_full_precision", "pr50k3_full_recall"))
    # 24 reals and 32 generated images in row batches of 16: 2 + 2 radius launches and 2 + 2 membership launches, each on one tile
    tiles = [d[6] for v, d in seen if v == "single"]
    assert tiles == [0, 0, 1, 1, 0, 0, 1, 1] and not [v for v, _ in seen if v in ("split", "merge")]
