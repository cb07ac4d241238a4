"""bench.py's plain run end to end, in a process of its own: the result line's contract keys (``ms_per_step`` is the time
of ONE timed step), no side measurement without ``--full``, and ``--dump-outputs`` writes what the timed path computed -
the predictions of the last timed forward: the bits a launch group of the same seeded batch gives, within the oracle's
float32 noise of float64 truth."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gcnn_keras_amd import synth
from oracle import kgcnn_oracle as ko
from parity import assert_rows_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_predictions(tmp_path):
    out = tmp_path / "outputs"
    # 10 steps = two launch groups of five batches: the last step is the last member of a group launch
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 10 and line["warmup"] == 2 and line["unit"] == "edges/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    edges = line["config"]["edges"]
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(edges, rel=1e-9)
    for key in ("single_forward_latency_ms", "roofline", "cpu_baseline", "stream_fresh_batches", "config4_single_gpu"):
        assert key not in line
    assert sorted(os.listdir(out)) == ["predictions.npy"]
    got = np.load(out / "predictions.npy")
    assert got.dtype == np.float32 and got.shape == (128, 1)
    b = synth.qm9_like_batch(num_graphs=128, seed=1234)
    assert int(b["edge_splits"][-1]) == edges
    p = synth.schnet_params(seed=7)
    # bit for bit what the timed path computes: the last member of a launch group of five copies of the batch (the bench
    # keeps four groups in flight, whose node chains run on half the CUs: the same bits, tests/test_gpu_fullsize.py)
    from gcnn_keras_amd.engine import SchnetForward
    f = SchnetForward(p, depth=3, mode="fused", group=5)
    f.load_batch(b)
    same = f.replay_group(0)[-1].cpu().numpy()
    torch.cuda.set_stream(torch.cuda.default_stream())
    f.check_flags()
    assert np.array_equal(got, same)
    # and the oracle's: with the bench's Keras-default zero biases some graph rows of this batch cancel, so the float32
    # oracle itself is ~5e-4 from float64 there - the bar is that noise floor (stated here, as parity.py asks)
    ref32, ref64 = [ko.schnet_forward(ko.to_dtype(p, dt), ko.R(b["node_number"], b["node_splits"]),
                                      ko.R(b["node_coordinates"].astype(dt), b["node_splits"]),
                                      ko.R(b["edge_indices"], b["edge_splits"]), depth=3) for dt in (np.float32, np.float64)]
    assert_rows_close(got, ref32, ref64, cap=1e-3, what="bench.py --dump-outputs predictions vs the oracle")
