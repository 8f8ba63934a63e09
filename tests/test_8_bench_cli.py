"""bench.py's command line without a GPU: `--dump-outputs DIR` (what the timed path's last step returned, float32 / float64, <= 64 MB,
large planes as a seeded pixel sample + full plane sums) and a plain run's line (no side measurements without `--full`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_small_arrays_whole_and_samples_large_planes(tmp_path):
    bench = _bench_module()
    from psalm_amd.model import Instances
    g = torch.Generator().manual_seed(3)
    H = W = 512
    mask_pred = torch.randn(12, H, W, generator=g)                       # 12 MB as float32: over DUMP_FULL_BYTES -> sampled
    sem_seg = torch.randn(3, H, W, generator=g)                          # 3 MB: whole
    pan = torch.randint(0, 5, (H, W), generator=g, dtype=torch.int32)    # 2 MB as float64: whole
    res = {"mask_pred": mask_pred, "sem_seg": sem_seg,
           "instances": Instances((H, W), pred_masks=mask_pred[:2] > 0, scores=torch.rand(2, generator=g), pred_classes=torch.tensor([4, 1])),
           "panoptic_seg": (pan, [{"id": 1, "isthing": True, "category_id": 7}, {"id": 2, "isthing": False, "category_id": 0}])}
    bench.dump_outputs(res, str(tmp_path))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"mask_pred", "mask_pred__pixels", "mask_pred__plane_sum", "sem_seg", "instances_pred_masks", "instances_scores",
                        "instances_pred_classes", "panoptic_seg_0", "panoptic_seg_1"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES
    pix = got["mask_pred__pixels"].astype(np.int64)
    assert pix.shape == (bench.DUMP_PIXELS,) and np.all(np.diff(pix) > 0) and pix[-1] < H * W
    assert got["mask_pred"].shape == (12, bench.DUMP_PIXELS)
    assert np.array_equal(got["mask_pred"], mask_pred.reshape(12, -1).numpy()[:, pix])
    np.testing.assert_allclose(got["mask_pred__plane_sum"], mask_pred.reshape(12, -1).double().sum(1).numpy(), rtol=1e-12)
    assert np.array_equal(got["sem_seg"], sem_seg.numpy()) and got["sem_seg"].dtype == np.float32
    assert np.array_equal(got["panoptic_seg_0"], pan.numpy()) and got["panoptic_seg_0"].dtype == np.float64
    assert np.array_equal(got["instances_pred_masks"], (mask_pred[:2] > 0).numpy().astype(np.float32))
    assert np.array_equal(got["instances_pred_classes"], [4.0, 1.0])
    assert np.array_equal(got["panoptic_seg_1"], [[7, 1, 1], [0, 2, 0]])      # fields in sorted key order: category_id, id, isthing
    # the sample is fixed: a second dump of the same result is identical
    bench.dump_outputs(res, str(tmp_path / "again"))
    assert all(np.array_equal(np.load(tmp_path / "again" / (k + ".npy")), v) for k, v in got.items())


@pytest.mark.slow
def test_plain_run_line_and_dumped_outputs_do_not_depend_on_steps_emu(tmp_path):
    """`--emu` (host-emulated kernels, the tiny architecture): a plain run prints the headline line with no side measurement, `--steps`
    sets the timed steps, and the dumped outputs are the same for another number of steps / warm-up steps (seeded weights and inputs)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from ops_backend import make_ops
    make_ops("emu")                                   # build the host-emulation library once, here
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    lines = {}
    for steps, warmup in ((2, 1), (1, 0)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--emu", "--eager", "--precision", "fp32",
                            "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / f"s{steps}")],
                           capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[steps] = json.loads(r.stdout.strip().splitlines()[-1])
    for steps, line in lines.items():
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["dtype"] == "fp32"
        assert abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-2 * line["value"] + 1e-3
        for side in ("gpu_ms_per_step", "roofline", "cpu_baseline", "parity_vs_cpu_oracle", "other_modes", "two_in_flight"):
            assert line[side] is None, side
    names = sorted(os.listdir(tmp_path / "s2"))
    assert names == sorted(os.listdir(tmp_path / "s1")) and "mask_pred.npy" in names and "sem_seg.npy" in names
    for n in names:
        a, b = np.load(tmp_path / "s2" / n), np.load(tmp_path / "s1" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
