"""bench.py --dump-outputs on the host side: what dump_outputs() writes for whole and sampled frames, its size bound, and that the sample is
fixed (two builds of the project are compared output for output).  CPU tensors stand in for the device buffers."""
import numpy as np
import torch

import bench


def _dump(tmp_path, name, frames, budget):
    old = bench.DUMP_BYTES
    bench.DUMP_BYTES = budget
    try:
        out = tmp_path / name
        bench.dump_outputs(torch, str(out), frames)
        return out
    finally:
        bench.DUMP_BYTES = old


def test_small_frames_are_written_whole_as_float32(tmp_path):
    f32 = torch.arange(40 * 30 * 3, dtype=torch.float32) / 7.0
    u8 = torch.arange(5 * 4 * 3, dtype=torch.uint8)
    u16 = torch.from_numpy(np.array([0, 1, 40000, 65535] * 15, dtype=np.uint16).view(np.int16))   # the 16-bit output's int16 buffer
    out = _dump(tmp_path, "d", [("frame0", f32, 40, 3), ("frame1", u8, 5, 3), ("frame2", u16, 5, 3)], 1 << 20)
    assert sorted(p.name for p in out.iterdir()) == ["frame0.npy", "frame1.npy", "frame2.npy"]
    a, b, c = (np.load(out / ("frame%d.npy" % i)) for i in range(3))
    assert a.dtype == b.dtype == c.dtype == np.float32
    assert a.shape == (40, 30, 3) and np.array_equal(a.ravel(), f32.numpy())
    assert b.shape == (5, 4, 3) and np.array_equal(b.ravel(), np.arange(60, dtype=np.float32))
    assert np.array_equal(c.ravel(), np.array([0, 1, 40000, 65535] * 15, dtype=np.float32))


def test_large_frames_are_a_fixed_row_sample_within_the_budget(tmp_path):
    H, W = 500, 64
    frames = [("frame%d" % i, torch.rand(H * W * 3, generator=torch.Generator().manual_seed(i)), H, 3) for i in range(2)]
    budget = 200 * 1024
    outs = [_dump(tmp_path, "d%d" % k, frames, budget) for k in range(2)]
    for out in outs:
        total = sum(np.load(out / ("frame%d.npy" % i)).nbytes for i in range(2))
        assert 0 < total <= budget
        for name, t, rows, _ in frames:
            a = np.load(out / (name + ".npy"))
            idx = np.load(out / (name + "_rows.npy"))
            assert idx.dtype == np.float64 and idx[0] == 0 and idx[-1] == rows - 1 and np.all(np.diff(idx) > 0)
            assert a.shape == (idx.size, W, 3) and np.array_equal(a, t.view(rows, W, 3).numpy()[idx.astype(np.int64)])
    for name in ("frame0.npy", "frame0_rows.npy", "frame1.npy"):
        assert np.array_equal(np.load(outs[0] / name), np.load(outs[1] / name))


def test_a_row_larger_than_the_budget_is_cut_to_it(tmp_path):
    t = torch.arange(3 * 1000 * 3, dtype=torch.float32)
    out = _dump(tmp_path, "d", [("frame0", t, 3, 3)], 4 * 300)
    a = np.load(out / "frame0.npy")
    assert a.nbytes <= 4 * 300 and np.array_equal(a.ravel(), np.arange(a.size, dtype=np.float32))
    assert np.array_equal(np.load(out / "frame0_rows.npy"), [0.0])
