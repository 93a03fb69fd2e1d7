"""RTPT_FLAG_EXT_SMOOTH_GUIDE restated in numpy, for test_guide_normals_*.py: the guide normal K0 writes into the per-pixel normal plane
(csrc/shading_normal.hpp, G1-G5), K0's pixel-centre rays and per-id normal table, and the per-pixel-normal form of the filter's float64
restatement.

The expectation of K0's plane is built from pieces the other tests already hold to the device bit for bit: path_walker.closest_hits on
K0's rays for the id and the barycentrics b1 = -u / ad, b2 = v / ad; b0 = 1 - b1 - b2 as gbuffer_pixel forms it; normal_paths.interpolate
for rules 1 to 3; the contract's cross / normalize / dot for k_lut's table."""
import numpy as np

import normal_paths as NP
import path_walker as WK
from dielectric_scenes import _contract, dot, fma, normalize

F32, U32 = np.float32, np.uint32
SMOOTH_GUIDE = 0x100000
SHAPE = (70, 19)        # one full 64-pixel tile column and a partial one; two 8-row comb chunks and a partial one


# ------------------------------------------------------------------------------------------ the filter, per-pixel normals
def atrous_once_numpy_px(dtype, img, depth, normals_px, stride, sigma_n=128, sigma_z=1.0, sigma_l=4.0):
    """filter_planes.atrous_once_numpy with the normal of a pixel taken from the plane normals_px [H, W, 3] instead of a per-id table:
    with normals_px = normals[ids] it is that function, operation for operation.  Returns [H, W, 3]."""
    H, W = np.asarray(depth).shape
    c = np.asarray(img[..., :3], dtype)
    d = np.asarray(depth, dtype)
    n = np.asarray(normals_px, dtype)[..., :3]
    num = np.zeros((H, W, 3), dtype)
    den = np.zeros((H, W), dtype)
    yy, xx = np.mgrid[0:H, 0:W]
    h = dtype(1) / dtype(9)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            qx = np.clip(xx + i * stride, 0, W - 1)
            qy = np.clip(yy + j * stride, 0, H - 1)
            cq, dq, nq = c[qy, qx], d[qy, qx], n[qy, qx]
            wn = np.maximum(dtype(0), (n * nq).sum(-1))
            assert sigma_n == 128
            for _ in range(7):
                wn = (wn * wn).astype(dtype)
            wd = np.exp(-np.abs(d - dq) / dtype(sigma_z))
            wl = np.exp(-np.sqrt(((c - cq) ** 2).sum(-1)) / dtype(sigma_l))
            hw = (h * ((wn * wd) * wl)).astype(dtype)
            num += hw[..., None] * cq
            den += hw
    return num / den[..., None]


# ------------------------------------------------------------------------------------------ K0's rays and table
def k0_rays(O, view, proj, W, H):
    """(origin [3], directions [H, W, 3]) float32 of K0's pixel-centre rays (gbuffer_tile.hpp: gbuffer_pixel, kernels.hip: k_ray_tables)
    for column-major view / proj"""
    V = np.asarray(view, F32).ravel()
    P = np.asarray(proj, F32).ravel()
    c = [V[0:3], V[4:7], V[8:11]]
    t = V[12:15]
    org = np.array([-dot(O, c[k][None], t[None])[0] for k in range(3)], F32)
    fw, fh = F32(W), F32(H)
    dvx = ((fma(O, F32(2.0), (np.arange(W, dtype=F32) + F32(0.5)).astype(F32), -fw) / fw).astype(F32) / P[0]).astype(F32)
    dvy = ((fma(O, F32(2.0), (np.arange(H, dtype=F32) + F32(0.5)).astype(F32), -fh) / fh).astype(F32) / P[5]).astype(F32)
    dv = np.stack([np.broadcast_to(dvx[None, :], (H, W)), np.broadcast_to(dvy[:, None], (H, W)), np.full((H, W), -1.0, F32)], -1).reshape(-1, 3)
    d = normalize(O, np.stack([dot(O, np.broadcast_to(c[k], dv.shape), dv) for k in range(3)], 1))
    return org, d.reshape(H, W, 3)


def powi128(x):
    """exact::powi(x, 128): seven squarings"""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        for _ in range(7):
            x = (x * x).astype(F32)
    return x


def self_weight(O, n):
    """powi(max(0, dot(n, n)), 128) per row of n [k, 3]; glsl_max(0, NaN) is 0"""
    d = dot(O, n, n)
    with np.errstate(invalid="ignore"):
        return powi128(np.where(d > 0, d, F32(0)).astype(F32))


def normal_table(O, tris):
    """[(T + 1), 4] float32: k_lut's normal_tab of posed triangles [T, 9] — normalize(cross(v1 - v0, v2 - v0)) and the self weight;
    id 0: (0, 0, 1)"""
    v = np.asarray(tris, F32).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        n = normalize(O, _contract(O, "cross", (v[:, 1] - v[:, 0]).astype(F32), (v[:, 2] - v[:, 0]).astype(F32)))
    n = np.concatenate([np.array([[0, 0, 1]], F32), n])
    return np.concatenate([n, self_weight(O, n)[:, None]], 1).astype(F32)


# ------------------------------------------------------------------------------------------ G1-G5
def guide32(O, nrm, n_base, hid, b0, b1, b2, ng):
    """G1-G5 for hits on posed triangles hid (0-based) with K0's barycentrics; ng [k, 3] = xyz(normal_tab[hid + 1]).
    (ns [k, 3] — ng where G4 keeps the table's cell —, guided [k])"""
    hid = np.asarray(hid, np.int64)
    ns, guided = np.array(ng, F32), np.zeros(len(hid), bool)
    t, i = hid % n_base, hid // n_base
    sel = np.flatnonzero(np.asarray(nrm.tri_smooth)[t] != 0)
    if len(sel):
        n9 = np.asarray(nrm.tri_normals, F32).reshape(-1, 9)[t[sel]]
        n, ok = NP.interpolate(O, n9[:, 0:3], n9[:, 3:6], n9[:, 6:9], b0[sel], b1[sel], b2[sel], np.asarray(nrm.cof, F32)[i[sel]])
        ok = ok & (n != 0).any(1)                      # G4: the zero vector of an overflowed |w|^2
        with np.errstate(invalid="ignore"):
            n = np.where((dot(O, n, ns[sel]) < 0)[:, None], -n, n).astype(F32)
        ns[sel[ok]] = n[ok]
        guided[sel[ok]] = True
    return ns, guided


def guide64(nrm, n_base, hid, b0, b1, b2, ng):
    """the same in float64 from the float32 operands: (ns64 [k, 3], the dot G5 tests [k], finite [k]) for hits on SMOOTH records"""
    hid = np.asarray(hid, np.int64)
    t, i = hid % n_base, hid // n_base
    n9 = np.asarray(nrm.tri_normals, np.float64).reshape(-1, 3, 3)[t]
    b = np.stack([b0, b1, b2], 1).astype(np.float64)
    with np.errstate(all="ignore"):
        m = (b[:, :, None] * n9).sum(1)
        w = np.einsum("krc,kc->kr", np.asarray(nrm.cof, np.float64)[i], m)
        ns = w / np.linalg.norm(w, axis=1)[:, None]
        flip = (ns * np.asarray(ng, np.float64)).sum(1)
        ns = np.where((flip < 0)[:, None], -ns, ns)
    return ns, flip, np.isfinite(ns).all(1)


def k0_hits(O, tris, view, proj, W, H, tmax):
    """K0 of posed triangles [T, 9]: (ids [H, W] uint32, b0, b1, b2 [H, W] float32)"""
    org, d = k0_rays(O, view, proj, W, H)
    ids, _, b1, b2 = WK.closest_hits(O, tris, np.broadcast_to(org, (H * W, 3)), d.reshape(-1, 3), tmax)
    b0 = ((F32(1.0) - b1).astype(F32) - b2).astype(F32)
    return ids.reshape(H, W), b0.reshape(H, W), b1.reshape(H, W), b2.reshape(H, W)


def guide_plane(O, tris, nrm, n_base, hits, guide=True):
    """[H, W, 4] float32: the per-pixel normal plane K0 writes for `hits` (k0_hits) — normal_tab[id] everywhere without the switch"""
    ids, b0, b1, b2 = hits
    tab = normal_table(O, tris)
    cells = tab[ids.astype(np.int64)].copy()
    if not guide or nrm is None:
        return cells, np.zeros(ids.shape, bool)
    hit = ids > 0
    ns, guided = guide32(O, nrm, n_base, ids[hit].astype(np.int64) - 1, b0[hit], b1[hit], b2[hit], cells[hit][:, :3])
    new = cells[hit]
    new[guided, :3] = ns[guided]
    new[guided, 3] = self_weight(O, ns[guided])
    cells[hit] = new
    mask = np.zeros(ids.shape, bool)
    mask[hit] = guided
    return cells, mask


# ------------------------------------------------------------------------------------------ injected normal planes
PLANE_KINDS = ("unit", "nan", "zero", "length2", "opposite", "denormal")


def normal_plane(kind, W, H, seed=0):
    """[H, W, 4] float32 cells (n.xyz, self weight as K0 would form it... or not: the kernels take the fourth word as it stands) of one
    hostile class.  unit: unit normals varying per pixel inside a cone of 12 degrees; nan: that with NaN components planted; zero: with
    zero vectors; length2: every normal of length 2; opposite: neighbours alternate between n and -n; denormal: components near 1e-40"""
    rng = np.random.default_rng([91, PLANE_KINDS.index(kind), W, H, seed])
    th = np.radians(12.0) * np.sqrt(rng.random((H, W)))
    ph = rng.uniform(0.0, 2.0 * np.pi, (H, W))
    n = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1)
    if kind == "length2":
        n = 2.0 * n
    elif kind == "opposite":
        yy, xx = np.mgrid[0:H, 0:W]
        n = np.where((((xx + yy) & 1) == 1)[..., None], -n, n)
    elif kind == "denormal":
        n = n * 1e-40
    n = n.astype(F32)
    if kind == "nan":
        for k, (y, x) in enumerate([(0, 0), (H - 1, W - 1), (H // 2, W // 2), (H // 3, 2 * W // 3), (2 * H // 3, W // 3), (1, W // 2), (H // 2, 1)]):
            n[y, x, k % 3] = np.nan
    elif kind == "zero":
        for (y, x) in [(0, W - 1), (H - 1, 0), (H // 2, W // 2), (H // 3, W // 3), (2 * H // 3, 2 * W // 3)]:
            n[y, x] = 0.0
    with np.errstate(all="ignore"):
        d = (n.astype(np.float64) ** 2).sum(-1).astype(F32)
        w = powi128(np.where(d > 0, d, F32(0)).astype(F32))
    cells = np.concatenate([n, w[..., None]], -1).astype(F32)
    cells.setflags(write=False)
    return cells
