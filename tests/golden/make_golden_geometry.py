"""Golden vectors for the overlapping / anisotropic convolution geometries (build container only, like make_golden.py).

    python tests/golden/make_golden_geometry.py

Runs the REAL reference's `spdownsample` and `conv3d` (torchsparse v1.4.0 through _ref_env.setup_torchsparse(), on the CPU) on one
small two-scene batch and stores inputs + results in ops_geometry.npz.  Data only; this file holds no reference code.

  (a) kernel 3 / stride 2                     (b) kernel 3 / stride (2, 2, 1)
  (c) kernel 3 / stride 2 on the output of (a): input tensor stride 2
  (d) kernel (3, 1, 3) / stride (2, 1, 2)
  (e) kernels (1, 3, 3), (3, 1, 3), (1, 1, 3) at stride 1

Per geometry: output coordinates, nbmaps / nbsizes of the cached map, y = conv(x) for 8 -> 16 channels, and gx / gw for a fixed
gy; for (a)-(d) also the transposed convolution back up through the cached map (yu and the gradients of x and both kernels).
Arrays of one shape are shared to keep the file small: `x` and `gyu` by every geometry over the batch's own coordinates, `e_gy`
by the three kernels of (e); (c), over the coordinates of (a), has its own `c_x` / `c_gyu`.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import _ref_env  # noqa: E402

torch.set_num_threads(1)
BACKEND_DESC = _ref_env.setup_torchsparse()
import torchsparse.nn.functional as F  # noqa: E402
from torchsparse import SparseTensor  # noqa: E402

C_IN, C_OUT = 8, 16
STRIDED = {"a": ((3, 3, 3), (2, 2, 2)), "b": ((3, 3, 3), (2, 2, 1)), "c": ((3, 3, 3), (2, 2, 2)), "d": ((3, 1, 3), (2, 1, 2))}
PLAIN = {"e133": (1, 3, 3), "e313": (3, 1, 3), "e113": (1, 1, 3)}


def make_coords():
    """Two scenes of ~270 voxels: scene 0 in [3, 14)^3, scene 1 in [-2, 9)^3 - the batch-wide minimum is scene 1's and negative.
    One voxel sits alone at the global minimum (-2, -2, -2): nothing else of scene 1 within two cells of it."""
    rs = np.random.RandomState(7)
    scenes = []
    for b, lo in enumerate((3, -2)):
        cells = np.stack(np.unravel_index(rs.choice(11 ** 3, 300, replace=False), (11, 11, 11)), 1) + lo
        if b == 1:
            cells = cells[np.abs(cells - lo).max(1) > 2]
            cells = np.concatenate([cells[:150], [[lo, lo, lo]], cells[150:]])
        cells = cells[:270]
        scenes.append(np.concatenate([cells, np.full((len(cells), 1), b)], 1))
    return np.concatenate(scenes).astype(np.int32)


def run_strided(out, tag, coords, in_stride, kernel, stride, x, gyu, g):
    k = int(np.prod(kernel))
    n = coords.shape[0]
    x = x.clone().requires_grad_()
    w = (torch.randn(k, C_IN, C_OUT, generator=g) * 0.2).requires_grad_()
    wu = (torch.randn(k, C_OUT, C_IN, generator=g) * 0.2).requires_grad_()
    st = SparseTensor(x, torch.from_numpy(coords), in_stride)
    st.cmaps[st.stride] = st.coords
    y = F.conv3d(st, w, kernel, stride=stride)
    gy = torch.randn(y.F.shape, generator=g)
    gx, gw = torch.autograd.grad(y.F, (x, w), gy, retain_graph=True)
    yu = F.conv3d(y, wu, kernel, stride=stride, transposed=True)
    assert yu.C is st.coords and yu.F.shape == (n, C_IN)
    ugx, ugw, ugwu = torch.autograd.grad(yu.F, (x, w, wu), gyu)
    nbmaps, nbsizes, sizes = st.kmaps[(st.stride, kernel, stride, (1, 1, 1))]
    assert sizes == (n, y.C.shape[0])
    out.update({f"{tag}_coords_in": coords, f"{tag}_coords": y.C.numpy().astype(np.int32),
                f"{tag}_nbmaps": nbmaps.numpy().astype(np.int32), f"{tag}_nbsizes": nbsizes.numpy().astype(np.int32),
                f"{tag}_w": w.detach().numpy(), f"{tag}_wu": wu.detach().numpy(),
                f"{tag}_y": y.F.detach().numpy(), f"{tag}_gy": gy.numpy(), f"{tag}_gx": gx.numpy(), f"{tag}_gw": gw.numpy(),
                f"{tag}_yu": yu.F.detach().numpy(), f"{tag}_ugx": ugx.numpy(),
                f"{tag}_ugw": ugw.numpy(), f"{tag}_ugwu": ugwu.numpy()})
    return y.C.numpy().astype(np.int32)


def run_plain(out, tag, coords, kernel, x, gy, g):
    k = int(np.prod(kernel))
    x = x.clone().requires_grad_()
    w = (torch.randn(k, C_IN, C_OUT, generator=g) * 0.2).requires_grad_()
    st = SparseTensor(x, torch.from_numpy(coords), 1)
    y = F.conv3d(st, w, kernel)
    gx, gw = torch.autograd.grad(y.F, (x, w), gy)
    nbmaps, nbsizes, _ = st.kmaps[(st.stride, kernel, (1, 1, 1), (1, 1, 1))]
    out.update({f"{tag}_nbmaps": nbmaps.numpy().astype(np.int32), f"{tag}_nbsizes": nbsizes.numpy().astype(np.int32),
                f"{tag}_w": w.detach().numpy(), f"{tag}_y": y.F.detach().numpy(), f"{tag}_gx": gx.numpy(),
                f"{tag}_gw": gw.numpy()})


def main():
    out = {"backend": np.array(BACKEND_DESC)}
    coords = make_coords()
    out["coords"] = coords
    g = torch.Generator().manual_seed(9)
    n = coords.shape[0]
    x, gyu, e_gy = torch.randn(n, C_IN, generator=g), torch.randn(n, C_IN, generator=g), torch.randn(n, C_OUT, generator=g)
    out.update(x=x.numpy(), gyu=gyu.numpy(), e_gy=e_gy.numpy())
    down = {}
    for tag, (kernel, stride) in STRIDED.items():
        if tag == "c":
            src, in_stride = down["a"], (2, 2, 2)
            xs, gs = torch.randn(len(src), C_IN, generator=g), torch.randn(len(src), C_IN, generator=g)
            out.update(c_x=xs.numpy(), c_gyu=gs.numpy())
        else:
            src, in_stride, xs, gs = coords, (1, 1, 1), x, gyu
        down[tag] = run_strided(out, tag, src, in_stride, kernel, stride, xs, gs, g)
    for tag, kernel in PLAIN.items():
        run_plain(out, tag, coords, kernel, x, e_gy, g)
    path = os.path.join(HERE, "ops_geometry.npz")
    np.savez_compressed(path, **out)
    print("ops_geometry.npz:", coords.shape[0], "voxels ->", {t: c.shape[0] for t, c in down.items()}, "rows;",
          os.path.getsize(path) // 1024, "KiB; backend:", BACKEND_DESC)


if __name__ == "__main__":
    main()
