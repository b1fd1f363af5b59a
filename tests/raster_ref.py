"""numpy restatement of k_rasterize (topoflow-glacier_amd/csrc/tfg_raster.hpp),
driven by hydrofabric.polygon_tables' output: per row, each ring's crossings
are formed once per edge and row (not once per edge and cell, as
hydrofabric.rasterize_divides does), gathered in lists of at most `cap`
edges' crossings whose parities XOR, shell and holes combine per cell, and the
last polygon wins.  Also the synthetic cases the host and the GPU tests share.
"""

from __future__ import annotations

import numpy as np

CAP = 256  # the kernel's fill: one edge per lane of a workgroup


def rasterize(t, outside_id: int, cap: int = CAP) -> np.ndarray:
    """int32 [rows][nx] from PolygonTables `t`."""
    rows, nx = len(t.py), len(t.px)
    out = np.full((rows, nx), outside_id, dtype=np.int32)
    for r in range(rows):
        py = t.py[r]
        for p in range(len(t.poly_id)):
            r0, r1, c0, c1 = t.poly_box[p]
            if not r0 <= r < r1:
                continue
            inside = np.zeros(nx, dtype=bool)  # a polygon without rings covers nothing
            for k in range(t.poly_ring0[p], t.poly_ring0[p + 1]):
                par = np.zeros(nx, dtype=bool)
                for e0 in range(t.ring_edge0[k], t.ring_edge0[k + 1], cap):  # one fill of the list
                    a, b, c, d = t.edges[e0:min(e0 + cap, t.ring_edge0[k + 1])].T
                    cross = (b > py) != (d > py)
                    a, b, c, d = a[cross], b[cross], c[cross], d[cross]
                    xc = a + (py - b) * (c - a) / (d - b)
                    par ^= (np.count_nonzero(t.px[:, None] < xc[None, :], axis=1) & 1).astype(bool)
                inside = par if k == t.poly_ring0[p] else inside & ~par
            out[r, c0:c1][inside[c0:c1]] = t.poly_id[p]
    return out


def host_ids(divides, x0, y0, cell, ny, nx, outside_id: int) -> np.ndarray:
    """What every comparison is against: rasterize_divides with -1 -> outside_id."""
    from topoflow_glacier.hydrofabric import rasterize_divides

    r = rasterize_divides(divides, x0, y0, cell, ny, nx)
    return np.where(r < 0, outside_id, r).astype(np.int32)


# ---------------------------------------------------------------------------
# Synthetic cases: cell = 1 and x0 = y0 integral, so centres sit at .5 and every
# crossing of the shapes below is exact in fp64.  Shapes are given in grid
# coordinates (u right, v down from the upper-left corner) and mapped to x, y.
X0, Y0 = 10.0, 40.0


def _ring(uv) -> np.ndarray:
    uv = np.asarray(uv, dtype=np.float64)
    return np.stack([X0 + uv[:, 0], Y0 - uv[:, 1]], axis=1)


def _rect(u0, v0, u1, v1):
    return _ring([(u0, v0), (u1, v0), (u1, v1), (u0, v1)])


def _divides(*polygon_lists):
    from topoflow_glacier.hydrofabric import Divide

    return [Divide(f"s-{i}", 0.0, list(p)) for i, p in enumerate(polygon_lists)]


def comb(teeth: int, pitch: float = 2.3, width: float = 1.1):
    """A comb whose row through the teeth has 2 * teeth crossings."""
    uv = [(1.0, 4.6)]
    for k in range(teeth):
        u = 1.0 + pitch * k
        uv += [(u, 3.2), (u, 0.7), (u + width, 0.7), (u + width, 3.2)]
    uv.append((1.0 + pitch * (teeth - 1) + width, 4.6))
    return _ring(uv)


def circle(vertices: int, cu: float, cv: float, radius: float):
    th = 2 * np.pi * np.arange(vertices) / vertices
    return _ring(np.stack([cu + radius * np.cos(th), cv + radius * np.sin(th)], axis=1))


def _slanted(ny, nx):
    """A quadrilateral over part of an ny x nx grid, one vertex off the grid."""
    return _ring([(-0.7, -0.4), (0.81 * nx + 0.3, 0.1 * ny), (0.55 * nx, ny + 0.6), (0.12 * nx, 0.7 * ny + 0.2)])


def synthetic_cases() -> dict:
    """name -> (divides, ny, nx); every grid has x0, y0 = X0, Y0 and cell = 1."""
    a, b = _rect(3, 2, 15, 13), [_rect(1, 1, 9, 8), _rect(5, 5, 16, 12)]  # two divides that overlap
    b_hole = [_rect(5, 3, 17, 14), _rect(7, 4, 12, 9)]  # the later polygon's hole lies over the earlier divide
    tri = _ring([(2.5, 1.5), (9.5, 4.5), (4.5, 8.5)])  # vertices on cell centres
    box = _rect(11.5, 2.5, 17.5, 7.5)  # horizontal and vertical edges through centres
    closed = np.concatenate([tri, tri[:1]])
    closed[:, 1] -= 9.0  # the same ring, closed, below the open one
    cases = {
        "a-hole": (_divides([[_rect(2, 2, 20, 19), _rect(6, 7, 12, 13)]]), 24, 24),
        "b-multi-and-empty": (_divides([[_rect(1, 1, 6, 5)], [_rect(8, 2, 13, 9)]], [], [[_rect(3, 7, 7, 11)]]), 13, 17),
        "c-later-wins": (_divides([[a]], [b_hole]), 16, 19),
        "c-reversed": (_divides([b_hole], [[a]]), 16, 19),
        "c-overlap": (_divides([[b[0]]], [[b[1]]]), 14, 18),
        "d-on-centres": (_divides([[tri]], [[box]], [[closed]]), 20, 21),
        "e-off-grid": (_divides([[_ring([(-6, 7), (11, -5), (29, 8), (12, 21)])]], [[_rect(-4, -3, 3, 2)]],
                                [[_rect(30, 3, 40, 9)]], [[_rect(5, 20, 9, 26)]], [[_rect(18, 11, 27, 19)]]), 15, 23),
        "f-comb": (_divides([[comb(300)]]), 5, 700),
        "g-circle": (_divides([[circle(5000, 33.3, 31.8, 29.7)]]), 64, 67),
        "h-2x1032": (_divides([[_slanted(2, 1032)]]), 2, 1032),
    }
    for ny, nx in ((1, 1), (1, 257), (3, 5), (7, 1027)):
        cases[f"h-{ny}x{nx}"] = (_divides([[_slanted(ny, nx)]]), ny, nx)
    return cases
