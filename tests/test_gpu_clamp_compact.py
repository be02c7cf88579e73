"""ts_stage_clamp_compact on the device (-m gpu): the clamp of the fused clouds as a stable compaction (csrc/compact.hip) against
numpy's `pts[(pts[:, :3] >= lo[s]).all(1)]` - rows, labels, both sample columns and the counts per sample bit for bit, at the
sizes where the kernels change behaviour: around the 256-row block and the 64-lane wave, sample boundaries inside a block, samples
without rows, 1 and 64 samples, 4- and 5-column rows, rows equal to the minimum, NaN and infinities, many blocks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from taseg_amd import backend as B  # noqa: E402


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rule(pts, lab, sample, lo):
    """nuscenes_voxel_ms.py:122-125 for every sample of the batch at once"""
    with np.errstate(invalid="ignore"):
        keep = (pts[:, :3] >= lo[sample]).all(1) if len(pts) else np.zeros(0, dtype=bool)
    return pts[keep], lab[keep], sample[keep], np.bincount(sample[keep], minlength=len(lo)).astype(np.int64)


def run(pts, lab, sample, lo):
    """one call against the rule; returns the device tensors of the surviving rows"""
    want_pts, want_lab, want_s, want_counts = rule(pts, lab, sample, lo)
    out, out_lab, out_s, out_s32, counts = B.stage_clamp_compact(T(pts), T(lab), T(sample.astype(np.int32)), T(lo))
    assert out.shape == pts.shape and out.dtype == torch.float32 and out_lab.dtype == torch.int64
    assert out_s.dtype == torch.int64 and out_s32.dtype == torch.int32 and counts.dtype == torch.int64
    assert counts.tolist() == want_counts.tolist()
    m = int(want_counts.sum())
    assert m == len(want_pts)
    assert np.array_equal(bits(out[:m].cpu().numpy()), bits(want_pts))
    assert np.array_equal(out_lab[:m].cpu().numpy(), want_lab)
    assert np.array_equal(out_s[:m].cpu().numpy(), want_s) and np.array_equal(out_s32[:m].cpu().numpy(), want_s.astype(np.int32))
    return out[:m], out_lab[:m], out_s[:m], out_s32[:m], counts


def batch(rng, sizes, cols, p_keep=0.6):
    """rows of len(sizes) samples (sizes[b] rows each, ascending sample index); about p_keep of them inside their sample's corner"""
    n = int(sum(sizes))
    sample = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    lo = rng.uniform(-3, 3, (len(sizes), 3)).astype(np.float32)
    side = (1.0 - p_keep ** (1 / 3.0)) if p_keep < 1 else 0.0        # per coordinate: P(below the minimum)
    pts = rng.uniform(0, 1, (n, cols)).astype(np.float32)
    below = rng.uniform(size=(n, 3)) < side
    pts[:, :3] = lo[sample] + np.where(below, -1, 1) * rng.uniform(0.01, 5, (n, 3)).astype(np.float32)
    lab = rng.randint(0, 17, n).astype(np.int64)
    return pts.astype(np.float32), lab, sample, lo


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 513])
@pytest.mark.parametrize("cols", [4, 5])
def test_row_counts_at_the_block_size(n, cols):
    rng = np.random.RandomState(10 * n + cols)
    run(*batch(rng, [n], cols))                                          # one sample
    if n >= 3:
        run(*batch(rng, [n // 3, n - n // 3 - 1, 1], cols))              # boundaries inside blocks and waves
    pts, lab, sample, lo = batch(rng, [n], cols, p_keep=1.0)
    out = run(pts, lab, sample, lo)
    assert out[0].shape[0] == n                                          # all rows kept
    lo_high = lo + 100
    assert run(pts, lab, sample, lo_high)[0].shape[0] == 0               # none kept


def test_samples_without_rows_and_64_samples():
    rng = np.random.RandomState(3)
    for sizes in ([0, 300, 200], [300, 0, 200], [300, 200, 0], [0, 0, 5, 0], [0], [0, 0]):
        out = run(*batch(rng, sizes, 4))
        assert all(c == 0 for c, s in zip(out[4].tolist(), sizes) if s == 0)
    # 64 samples: a few rows each, so that one wave holds many samples; some of them empty
    sizes = [int(v) for v in rng.randint(0, 40, 64)]
    sizes[0], sizes[63], sizes[17] = 0, 0, 0
    run(*batch(rng, sizes, 5))
    sizes = [1] * 64                                                      # one wave, 64 samples
    run(*batch(rng, sizes, 4))
    with pytest.raises(ValueError):
        B.stage_clamp_compact(T(np.zeros((2, 4), np.float32)), T(np.zeros(2, np.int64)), T(np.zeros(2, np.int32)),
                              T(np.zeros((65, 3), np.float32)))


def test_rows_at_the_minimum_nan_and_infinities():
    rng = np.random.RandomState(5)
    pts, lab, sample, lo = batch(rng, [200, 330], 4)
    # rows equal to the minimum in one, two and all three coordinates: kept (`>=`)
    for i, k in ((0, 1), (1, 2), (2, 3), (250, 3), (251, 1)):
        pts[i, :3] = lo[sample[i]] + 1
        pts[i, :k] = lo[sample[i], :k]
    pts[3, :3] = np.nextafter(lo[0], np.float32(-np.inf))                # one ulp below: dropped
    pts[4, :3] = (lo[0, 0] + 1, lo[0, 1] + 1, np.nextafter(lo[0, 2], np.float32(-np.inf)))
    pts[10, 0], pts[11, 1], pts[12, 2] = np.nan, np.nan, np.nan          # NaN fails, as numpy's `>=`
    pts[13, :3] = np.inf                                                 # +inf >= anything finite
    pts[14, 0], pts[15, 2] = -np.inf, -np.inf
    pts[16, :3] = lo[0] + 1
    pts[16, 3] = np.nan                                                  # a NaN feature is no coordinate: the row stays, bits kept
    pts[300, :3] = (np.inf, lo[1, 1], lo[1, 2])
    pts[301, :3] = -0.0
    out = run(pts, lab, sample, lo)
    kept = (pts[:, :3] >= lo[sample]).all(1)
    assert kept[[0, 1, 2, 13, 16, 250, 251, 300]].all() and not kept[[3, 4, 10, 11, 12, 14, 15]].any()
    assert np.isnan(out[0].cpu().numpy()[:, 3]).sum() == 1
    # a minimum that is NaN or infinite: nothing of that sample passes a NaN, everything finite passes -inf
    lo2 = lo.copy()
    lo2[0, 1] = np.nan
    lo2[1] = -np.inf
    out = run(pts, lab, sample, lo2)
    assert out[4].tolist()[0] == 0 and out[4].tolist()[1] == 330 - int(np.isnan(pts[200:, :3]).any(1).sum())
    lo2[1] = np.inf
    assert run(pts, lab, sample, lo2)[4].tolist() == [0, 0]                # (row 300 is +inf in x only)


def test_many_blocks_twice_the_same_bits():
    rng = np.random.RandomState(9)
    sizes = [1000, 1, 0, 1777, 513, 255, 1300]                           # 4846 rows, 19 blocks, the last one partial
    for cols in (4, 5):
        pts, lab, sample, lo = batch(rng, sizes, cols)
        a = run(pts, lab, sample, lo)
        b = run(pts, lab, sample, lo)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    # 4-column rows that start 4 bytes off a 16-byte boundary take the plain-load path
    pts, lab, sample, lo = batch(rng, [300, 310], 4)
    flat = torch.zeros(4 * 610 + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(-1, 4)
    view.copy_(T(pts))
    assert view.data_ptr() % 16 == 4
    got = B.stage_clamp_compact(view, T(lab), T(sample.astype(np.int32)), T(lo))
    want = rule(pts, lab, sample, lo)
    m = len(want[0])
    assert got[4].tolist() == want[3].tolist() and np.array_equal(bits(got[0][:m].cpu().numpy()), bits(want[0]))


@pytest.mark.parametrize("n_blocks", [255, 256, 257, 513, 1000])
def test_block_counts_around_the_scan_chunk(n_blocks):
    """the scan's 256 threads own one block count each up to 256 blocks and several behind it (chunks of 2, 3 and 4 here; the last
    chunks partial or empty); the last block of rows is partial"""
    rng = np.random.RandomState(n_blocks)
    n = 256 * n_blocks - 5
    first = n // 5
    run(*batch(rng, [first, 0, n - first], 4))


def test_64_samples_over_257_blocks():
    """every wave of the scan's tally blocks sums a row"""
    rng = np.random.RandomState(64)
    n = 256 * 257 - 5
    sizes = [int(v) for v in rng.randint(500, 1500, 63)]
    sizes[11] = 0
    assert sum(sizes) < n
    run(*batch(rng, sizes + [n - sum(sizes)], 4))


def test_arguments_are_checked():
    pts, lab, s, lo = (T(np.zeros((4, 4), np.float32)), T(np.zeros(4, np.int64)), T(np.zeros(4, np.int32)), T(np.zeros((1, 3), np.float32)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        B.stage_clamp_compact(pts.cpu(), lab, s, lo)
    with pytest.raises(TypeError):
        B.stage_clamp_compact(pts.double(), lab, s, lo)
    with pytest.raises(TypeError):
        B.stage_clamp_compact(pts, lab.int(), s, lo)
    with pytest.raises(TypeError):
        B.stage_clamp_compact(pts, lab, s.long(), lo)
    with pytest.raises(ValueError):
        B.stage_clamp_compact(pts, lab[:3], s, lo)
    with pytest.raises(TypeError):
        B.stage_clamp_compact(pts[:, :2], lab, s, lo)
    # a view is made contiguous, as the neighbours do
    wide = T(np.arange(40, dtype=np.float32).reshape(4, 10))
    out = B.stage_clamp_compact(wide[:, :5], lab, s, T(np.full((1, 3), -1, np.float32)))
    assert out[4].tolist() == [4] and torch.equal(out[0], wide[:, :5].contiguous())
