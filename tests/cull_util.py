"""The block cull restated in numpy (volrend_amd/csrc/vr_internal.h "Block cull"): occupancy grid, boundary
cells, and the per-frame mask of 8x8 pixel blocks that ray generation may skip.

The rule, as the library applies it:
  * grid of 2^g cells per axis, g = min(7, depth of the deepest leaf); a cell is set when a leaf that overlaps it
    has sigma > 0 (a float compare: NaN, -0 and negative values do not count);
  * listed: the set cells with an unset or out-of-grid face neighbour;
  * a listed cell, centre c in tree space, is the sphere around (c - offset) / scale with the half-diagonal r of
    the cell's box in world space (times 1.0001); in camera space (X, Y, depth) it covers the pixels within
    rx = |fx| r sqrt(depth^2 + X^2) / (depth (depth - r)) * 1.05 + 1 of x = w/2 + fx X / depth (y alike, with
    y = h/2 - fy Y / depth), and every 8x8 block that rectangle touches is marked;
  * depth - r <= r / 100 with depth + r >= 0 marks the whole frame (the camera plane cuts or nearly touches the
    sphere); a sphere wholly behind the plane marks nothing.
This file computes in float64: it restates the rule, not its rounding -- the tests ask that no culled block of
this mask holds a hit, and that the library culls no block the oracle shows occupied."""
import numpy as np

from tests import query_util as qu

MAX_LEVELS = 7


def occupancy(tree):
    """-> (g, bool [2^g, 2^g, 2^g]) of a tree with N == 2."""
    assert tree.N == 2
    corners, sizes, depths, slots = qu.leaf_boxes(tree)
    g = min(MAX_LEVELS, int(depths.max()) + 1)
    n = 1 << g
    sigma = tree.data.reshape(-1, tree.data_dim)[slots, -1].astype(np.float32)
    grid = np.zeros((n, n, n), dtype=bool)
    for c, s in zip(corners[sigma > 0], sizes[sigma > 0]):
        lo = np.floor(c * n + 1e-9).astype(int)
        e = max(1, int(round(s * n)))
        grid[lo[0]:lo[0] + e, lo[1]:lo[1] + e, lo[2]:lo[2] + e] = True
    return g, grid


def boundary_cells(grid):
    """-> int [m, 3]: the set cells with an unset or out-of-grid face neighbour."""
    p = np.pad(grid, 1, constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] &
             p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return np.argwhere(grid & ~inner)


def block_mask(tree, transform, w, h, fx, fy=None):
    """-> bool [ceil(h / 8), ceil(w / 8)]: True = the block is marked (not culled)."""
    fy = fx if fy is None else fy
    g, grid = occupancy(tree)
    cells = boundary_cells(grid)
    nbx, nby = (w + 7) // 8, (h + 7) // 8
    mask = np.zeros((nby, nbx), dtype=bool)
    if len(cells) == 0:
        return mask
    tr = np.asarray(transform, np.float64)
    R = tr[:9].reshape(3, 3)  # rows: the camera's right, up, back in world space
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-4:
        mask[:] = True
        return mask
    scale, offset = np.asarray(tree.invradius3, np.float64), np.asarray(tree.offset, np.float64)
    cell = 1.0 / (1 << g)
    r = np.sqrt(((0.5 * cell / scale) ** 2).sum()) * 1.0001
    world = ((cells + 0.5) * cell - offset) / scale
    cam = (world - tr[9:12]) @ R.T
    X, Y, depth = cam[:, 0], cam[:, 1], -cam[:, 2]
    near = ~(depth - r > 0.01 * r)
    if (near & ~(depth + r < 0)).any():
        mask[:] = True
        return mask
    X, Y, depth = X[~near], Y[~near], depth[~near]
    inv = 1.0 / (depth * (depth - r))
    rx = abs(fx) * r * np.sqrt(depth ** 2 + X ** 2) * inv * 1.05 + 1.0
    ry = abs(fy) * r * np.sqrt(depth ** 2 + Y ** 2) * inv * 1.05 + 1.0
    px, py = 0.5 * w + fx * X / depth, 0.5 * h - fy * Y / depth
    x0 = np.floor(np.maximum((px - rx) / 8, 0)).astype(int)
    x1 = np.floor(np.minimum((px + rx) / 8, nbx - 1)).astype(int)
    y0 = np.floor(np.maximum((py - ry) / 8, 0)).astype(int)
    y1 = np.floor(np.minimum((py + ry) / 8, nby - 1)).astype(int)
    for a, b, c, d in zip(x0, x1, y0, y1):
        if a <= b and c <= d:
            mask[c:d + 1, a:b + 1] = True
    return mask


def hit_blocks(hits):
    """-> bool [ceil(h / 8), ceil(w / 8)] from the oracle's per-pixel hit map: the block holds a pixel with a hit."""
    h, w = hits.shape
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    p = np.zeros((nby * 8, nbx * 8), dtype=bool)
    p[:h, :w] = hits > 0
    return p.reshape(nby, 8, nbx, 8).any(axis=(1, 3))
