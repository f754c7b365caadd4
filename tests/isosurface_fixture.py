"""Brute-force float64 statement of the isosurface rules of include/mipnerf_hip.h (marching tetrahedra on the Kuhn split), numpy only,
vectorised over cells -- the comparator of the extraction kernels, written from the rules and not from the kernels:

  - a lattice point is inside when f > threshold (NaN and a tie are outside);
  - every cell is cut into the six tetrahedra (c, c + e_p0, c + e_p0 + e_p1, c + (1,1,1)), p over the permutations of the axes;
  - one vertex per lattice edge whose ends differ, at p_in + t (p_out - p_in), t = (threshold - f_in) / (f_out - f_in), 0.5 when not finite;
  - vertices sorted by (smaller end, larger end) of their edge (flat index (k ny + j) nx + i);
  - winding FROM THE EDGE MIDPOINTS: the triangle through the midpoints of its three edges is never degenerate, and its normal must point
    from the inside end to the outside end of its first edge;
  - normals: -grad f normalised, central differences at the two ends (one-sided on the box), interpolated with t; 0 where zero / not finite.
"""
import itertools

import numpy as np

PERMUTATIONS = list(itertools.permutations(range(3)))


def lattice_positions(shape, lo, hi):
    """[Z*Y*X, 3] float64 positions (x, y, z) of the lattice points, flat index (k Y + j) X + i."""
    Z, Y, X = shape
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    ijk = np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    h = (hi - lo) / (np.array([X, Y, Z]) - 1)
    return lo + ijk * h, h


def lattice_gradient(f, h):
    """[Z*Y*X, 3] float64 (d/dx, d/dy, d/dz): central differences, one-sided on the faces of the box."""
    with np.errstate(all="ignore"):
        gz, gy, gx = np.gradient(f.astype(np.float64), h[2], h[1], h[0], edge_order=1)
    return np.stack([gx, gy, gz], -1).reshape(-1, 3)


def marching_tets(f, thr, lo, hi):
    """f [Z, Y, X]; returns a dict: vertices [V, 3] float64, normals [V, 3] float64, faces [F, 3] int64, edges [V, 2] int64 = flat indices
    of the (inside, outside) ends of each vertex's lattice edge, weak [V] bool = the interpolated gradient is shorter than 1e-3 of the
    longer end gradient (the two ends cancel, nearly or exactly: neither the direction of such a normal nor whether it is exactly zero is
    comparable across precisions)."""
    f = np.asarray(f)
    Z, Y, X = f.shape
    n = Z * Y * X
    idx = np.arange(n).reshape(Z, Y, X)
    pos, h = lattice_positions(f.shape, lo, hi)
    fv = f.reshape(-1).astype(np.float64)
    inside = fv > thr

    def corner(d):          # lattice ids of corner d = (dx, dy, dz) of every cell
        dx, dy, dz = d
        return idx[dz:Z - 1 + dz, dy:Y - 1 + dy, dx:X - 1 + dx].reshape(-1)

    tris = []               # [m, 3, 2] edges (a, b) of triangles, as corner pairs
    for perm in PERMUTATIONS:
        d0 = np.zeros(3, int)
        d1 = d0.copy(); d1[perm[0]] = 1
        d2 = d1.copy(); d2[perm[1]] = 1
        T = np.stack([corner(d) for d in (d0, d1, d2, np.ones(3, int))], 1)      # [cells, 4]
        ins = inside[T]
        cnt = ins.sum(1)
        for k in (1, 3):
            m = cnt == k
            if m.any():
                t = T[m]
                s = ins[m] if k == 1 else ~ins[m]
                a = t[s]                                                        # the lone corner
                o = t[~s].reshape(-1, 3)
                tris.append(np.stack([np.repeat(a[:, None], 3, 1), o], -1))
        m = cnt == 2
        if m.any():
            t, s = T[m], ins[m]
            a, o = t[s].reshape(-1, 2), t[~s].reshape(-1, 2)
            q = [np.stack([a[:, 0], o[:, 0]], -1), np.stack([a[:, 0], o[:, 1]], -1), np.stack([a[:, 1], o[:, 1]], -1),
                 np.stack([a[:, 1], o[:, 0]], -1)]
            tris.append(np.stack([q[0], q[1], q[2]], 1))
            tris.append(np.stack([q[0], q[2], q[3]], 1))
    if not tris:
        z3 = np.zeros((0, 3))
        return dict(vertices=z3, normals=z3.copy(), faces=np.zeros((0, 3), np.int64), edges=np.zeros((0, 2), np.int64),
                    weak=np.zeros(0, bool))
    E = np.concatenate(tris, 0)                                                   # [F, 3, 2]
    a, b = E[..., 0], E[..., 1]
    swap = ~inside[a]
    e_in, e_out = np.where(swap, b, a), np.where(swap, a, b)
    # winding from the edge midpoints
    M = 0.5 * (pos[e_in] + pos[e_out])
    nrm = np.cross(M[:, 1] - M[:, 0], M[:, 2] - M[:, 0])
    flip = (nrm * (pos[e_out[:, 0]] - pos[e_in[:, 0]])).sum(1) < 0
    key = np.minimum(a, b) * n + np.maximum(a, b)
    uk, first, inv = np.unique(key.reshape(-1), return_index=True, return_inverse=True)
    faces = inv.reshape(-1, 3).copy()
    faces[flip] = faces[flip][:, ::-1]
    v_in, v_out = e_in.reshape(-1)[first], e_out.reshape(-1)[first]
    with np.errstate(all="ignore"):
        t = (thr - fv[v_in]) / (fv[v_out] - fv[v_in])
    t = np.where(np.isfinite(t), t, 0.5)[:, None]
    vertices = pos[v_in] + t * (pos[v_out] - pos[v_in])
    grad = lattice_gradient(f, h)
    with np.errstate(all="ignore"):
        g = grad[v_in] + t * (grad[v_out] - grad[v_in])
        big = np.abs(g).max(1)
        ok = np.isfinite(g).all(1) & (big > 0)
        gs = np.where(ok[:, None], g / np.where(ok, big, 1.0)[:, None], 0.0)
        length = np.linalg.norm(gs, axis=1)
        normals = np.where(ok[:, None], -gs / np.where(ok, length, 1.0)[:, None], 0.0)
        ends = np.maximum(np.linalg.norm(grad[v_in], axis=1), np.linalg.norm(grad[v_out], axis=1))
        weak = np.isfinite(g).all(1) & np.isfinite(ends) & (np.linalg.norm(g, axis=1) < 1e-3 * ends)
    return dict(vertices=vertices, normals=normals, faces=faces.astype(np.int64), edges=np.stack([v_in, v_out], -1).astype(np.int64),
                weak=weak)


# ---- first-principle helpers on any (vertices, faces) ------------------------------------------------------------------------
def _half_edges(faces):
    faces = np.asarray(faces, np.int64)
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)


def is_closed(faces):
    """every undirected edge is in exactly two faces"""
    e = np.sort(_half_edges(faces), 1)
    if not len(e):
        return True
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return bool((cnt == 2).all())


def directed_edges_unique(faces):
    """every directed edge occurs at most once (holds for open meshes too)"""
    e = _half_edges(faces)
    return len(np.unique(e, axis=0)) == len(e)


def is_oriented(faces):
    """every directed edge occurs once and its reverse occurs"""
    e = _half_edges(faces)
    if not len(e):
        return True
    big = int(e.max()) + 1
    fwd, rev = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(rev))


def euler_characteristic(num_vertices, faces):
    e = np.sort(_half_edges(faces), 1)
    return int(num_vertices) - len(np.unique(e, axis=0)) + len(faces)


def enclosed_volume(vertices, faces):
    """divergence theorem, float64"""
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def zero_area_faces(vertices, faces):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    return int((np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1) == 0).sum())


def canonical_faces(faces, edges, n):
    """faces as sorted rows of lattice-edge keys ((smaller end) n + larger end), each rotated to start with its smallest key: equal for
    two meshes exactly when they have the same triangles with the same winding, whatever the vertex numbering."""
    edges = np.asarray(edges, np.int64)
    key = np.minimum(edges[:, 0], edges[:, 1]) * n + np.maximum(edges[:, 0], edges[:, 1])
    k = key[np.asarray(faces, np.int64)]
    if not len(k):
        return k.reshape(0, 3)
    r = np.argmin(k, 1)
    k = np.stack([k[np.arange(len(k)), (r + s) % 3] for s in range(3)], 1)
    return k[np.lexsort((k[:, 2], k[:, 1], k[:, 0]))]


# ---- the analytic test fields -------------------------------------------------------------------------------------------------
CENTRE = np.array([0.13, -0.07, 0.21])
SPHERE_R, TORUS_R, TORUS_A = 0.9, 0.8, 0.3
SPHERE_VOLUME = 4.0 / 3.0 * np.pi * SPHERE_R ** 3
TORUS_VOLUME = 2.0 * np.pi ** 2 * TORUS_R * TORUS_A ** 2


def _axes(n):
    g = np.linspace(-1.5, 1.5, n)
    return np.meshgrid(g, g, g, indexing="ij")          # z, y, x


def sphere_field(n):
    z, y, x = _axes(n)
    return (SPHERE_R ** 2 - ((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2)).astype(np.float32)


def torus_field(n):
    z, y, x = _axes(n)
    return (TORUS_A ** 2 - ((np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2) - TORUS_R) ** 2 + (z - CENTRE[2]) ** 2)).astype(np.float32)
