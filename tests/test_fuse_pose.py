"""The three pose-fuse entry points (ts_fuse_scan, ts_fuse_scans, ts_fuse_scans_batch) are ONE rule, sr_fuse_pose of
csrc/stage_rules.h: equal to each other bit for bit, and equal to numpy's float32 arithmetic restated here - every product and
every sum its own correctly rounded float32 operation, in k order.  The restatement itself is pinned on the host against the
pose-fused rows the reference's dataset code produced (tests/golden/multiscan.npz)."""
import numpy as np
import pytest
import torch

GRID_CAP = 4096 * 256                       # the launchers' grid cap in rows: one row more takes the grid-stride loop's second trip
ROWS = [1, 255, 256, 257, GRID_CAP + 1]
TWO_NANS = 200                              # the row where two different NaNs meet in an addition (same_bits)


def fuse_pose_np(points, pose0, pose):
    """float32 [n, 4] -> [n, 4]: new_j = ((h0 P[j][0] + h1 P[j][1]) + h2 P[j][2]) + h3 P[j][3] - Q[j][3], out_j = (new0 Q[0][j] +
    new1 Q[1][j]) + new2 Q[2][j]; numpy's float32 multiply and add are separate, correctly rounded operations"""
    P, Q = np.asarray(pose, dtype=np.float32), np.asarray(pose0, dtype=np.float32)
    h = [points[:, 0], points[:, 1], points[:, 2], np.ones(points.shape[0], dtype=np.float32)]
    new = []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(3):
            s = h[0] * P[j, 0]
            for k in (1, 2, 3):
                s = s + h[k] * P[j, k]
            new.append(s - Q[j, 3])
        out = points.copy()
        for j in range(3):
            out[:, j] = (new[0] * Q[0, j] + new[1] * Q[1, j]) + new[2] * Q[2, j]
    assert out.dtype == np.float32
    return out


def same_bits(a, b):
    """equal bit for bit; a NaN equals any NaN at the same place.  IEEE 754 leaves open which of two NaN operands an addition
    returns, and the compiler may commute an addition: in a row where the input's NaN (sign clear) meets the NaN that inf - inf
    makes (sign set, on the GPU as on x86) the result's sign is nobody's rule - measured on the MI355X, ts_fuse_scan and
    ts_fuse_scans return opposite signs there, before and after they shared sr_fuse_pose.  See TWO_NANS."""
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def test_numpy_restatement_equals_the_reference_rows(g_multiscan):
    g = g_multiscan
    Tn = int(g["T"])
    for b in range(2):
        fused = [fuse_pose_np(g[f"b{b}_points_t{t}"], g[f"b{b}_pose_t{Tn}"], g[f"b{b}_pose_t{t}"]) for t in range(Tn)]
        same_bits(np.concatenate(fused), g[f"b{b}_fused_all"])


def _pose(rng, yaw, t):
    """a rigid pose, perturbed: no entry is 0 or 1 and no product with it is exact"""
    c, s = np.cos(yaw), np.sin(yaw)
    m = np.array([[c, -s, 0, t[0]], [s, c, 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1]], dtype=np.float64)
    return (m + rng.uniform(1e-4, 1e-3, (4, 4))).astype(np.float32)


@pytest.fixture(scope="module")
def case():
    rng = np.random.RandomState(20)
    pts = (rng.standard_normal((GRID_CAP + 1, 4)) * np.array([30., 30., 2., 1.])).astype(np.float32)
    pts[3, 0], pts[5, 1], pts[7, 2] = np.nan, np.inf, -np.inf          # inside every row count >= 255 ...
    pts[9, :3], pts[11, 0] = [np.inf, np.inf, -np.inf], -np.nan         # (one source of NaN per row: its bits are defined)
    pts[TWO_NANS, :3] = [np.inf, -np.inf, np.nan]
    pts[GRID_CAP] = [np.nan, 1.5, -2.5, 0.25]                           # ... and in the second trip
    poses = np.stack([_pose(rng, 0.3 + 0.2 * i, rng.uniform(-20, 20, 3)) for i in range(6)])
    want = fuse_pose_np(pts, poses[0], poses[1])
    pts.setflags(write=False)
    want.setflags(write=False)
    return pts, poses, want


@pytest.mark.gpu
@pytest.mark.parametrize("n", ROWS)
def test_three_entry_points_one_rule(case, n):
    from taseg_amd import backend as B
    pts, poses, want = case
    p = torch.from_numpy(pts[:n].copy()).cuda()
    pose0, pose = torch.from_numpy(poses[0]).cuda(), torch.from_numpy(poses[1]).cuda()
    idx = torch.zeros(n, dtype=torch.int32, device="cuda")
    one = B.fuse_scan(p, pose0, pose).cpu().numpy()
    many = B.fuse_scans(p, idx, pose0, pose[None]).cpu().numpy()
    batch = B.fuse_scans_batch(p, idx, pose0[None], pose[None]).cpu().numpy()
    defined = np.arange(n) != TWO_NANS
    for other in (many, batch):
        assert np.array_equal(one.view(np.uint32)[defined], other.view(np.uint32)[defined])
        same_bits(one, other)
    same_bits(one, want[:n])


@pytest.mark.gpu
def test_fuse_scans_batch_three_scans_with_their_own_current_pose(case):
    from taseg_amd import backend as B
    pts, poses, _ = case
    lengths = [100, 257, 43]                                            # unequal, the second across a block boundary
    n = sum(lengths)
    idx = np.repeat(np.arange(3, dtype=np.int32), lengths)
    pose0s, hist = poses[[0, 2, 4]], poses[[1, 3, 5]]
    got = B.fuse_scans_batch(torch.from_numpy(pts[:n].copy()).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(pose0s).cuda(),
                             torch.from_numpy(hist).cuda()).cpu().numpy()
    at = 0
    for s, m in enumerate(lengths):
        same_bits(got[at:at + m], fuse_pose_np(pts[at:at + m], pose0s[s], hist[s]))
        one = B.fuse_scan(torch.from_numpy(pts[at:at + m].copy()).cuda(), torch.from_numpy(pose0s[s]).cuda(),
                          torch.from_numpy(hist[s]).cuda()).cpu().numpy()
        defined = np.arange(at, at + m) != TWO_NANS
        assert np.array_equal(one.view(np.uint32)[defined], got[at:at + m].view(np.uint32)[defined])
        same_bits(one, got[at:at + m])
        at += m
