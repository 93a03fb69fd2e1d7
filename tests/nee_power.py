"""The weighted light pick of next-event estimation (RTPT_FLAG_EXT_NEE_POWER; csrc/light_sample.hpp states the rules,
csrc/light_table.hip builds the table) restated in numpy for test_nee_power_*.py: the weights, the cumulative table, the pick,
the sample that takes the inverse of the pick's probability, hostile weights and the scenes.

Everything the device fixes is integer arithmetic or one correctly rounded float32 operation at a time, so numpy gives the same
bits: weights() is sample32's a2 times the largest |Ke| channel, table() the maximum, the quantisation and the integer running
sum, pick_power() the draw's 24 bits scaled into [0, S) and a binary search (numpy's searchsorted, side="right": the smallest i
with C_i > t).  tests/path_walker.py walks the paths with the weighted pick and inv_p where `power`; with `power` off it takes the
uniform pick, which test_nee_power_cpu.py asks for bit by bit against the recorded frames of the walker without the flag."""
import numpy as np

import nee_paths as NP
import nee_scenes as N
import pathtrace_scenes as P
from dielectric_scenes import dot, fma, normalize

F32, U32, U64 = np.float32, np.uint32, np.uint64
PICK_SCALE = F32(1 << 24)
WEIGHT_SCALE = F32(1 << 16)
BLOCK = 1024                                      # kLightTableBlock: entries a workgroup of the builder scans


# ------------------------------------------------------------------------------------------ weights and table
def weights(O, tris, rec, lights):
    """float32 [L]: w_i = a2_i * k_i of every entry of `lights` (id + 1 of posed triangles of tris [n, 9]; rec: one record per
    BASE triangle), before "counts as 0" """
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 9)
    rec = np.ascontiguousarray(rec, F32)
    ids = np.asarray(lights, np.int64) - 1
    t = tris[ids]
    with np.errstate(all="ignore"):
        e1, e2 = (t[:, 3:6] - t[:, 0:3]).astype(F32), (t[:, 6:9] - t[:, 0:3]).astype(F32)
        cr = N.cross(O, e1, e2)
        a2 = np.sqrt(dot(O, cr, cr)).astype(F32)
        ke = np.abs(rec[ids % len(rec), 4:7])
        k = ke[:, 0].copy()
        k = np.where(ke[:, 1] > k, ke[:, 1], k)
        k = np.where(ke[:, 2] > k, ke[:, 2], k)
        return (a2 * k).astype(F32)


def counted(w):
    """w where it is finite and > 0, else 0"""
    w = np.asarray(w, F32)
    with np.errstate(all="ignore"):
        return np.where((w > 0) & (w < np.inf), w, F32(0)).astype(F32)


def quantised(w):
    """uint32 [L]: q_i of the weights w"""
    w = counted(w)
    w_max = w.max() if len(w) else F32(0)
    if w_max == 0:
        return np.ones(len(w), U32)
    with np.errstate(all="ignore"):
        q = ((w / w_max).astype(F32) * WEIGHT_SCALE).astype(F32).astype(U32)
    return np.where(w > 0, np.maximum(q, 1), 0).astype(U32)


def table(w):
    """uint64 [L]: C_i = sum_{j <= i} q_j"""
    return np.cumsum(quantised(w).astype(U64), dtype=U64)


def scratch_bytes(n):
    """rt::light_table_scratch_bytes: the maximum's word (8), the workgroups' sums of every level of the scan (8 each), the
    weights (4 n)"""
    sums, m = 0, n
    while True:
        m = (m + BLOCK - 1) // BLOCK
        sums += m
        if m <= 1:
            break
    return 8 + 8 * sums + 4 * n


def pick_power(cdf, u_l):
    """(entry uint32 [k], inv_p float32 [k]) of draws u_l on the table cdf"""
    cdf = np.asarray(cdf, U64)
    S = cdf[-1]
    m = (np.asarray(u_l, F32) * PICK_SCALE).astype(F32).astype(U64)
    t = (m * S) >> U64(24)
    i = np.minimum(np.searchsorted(cdf, t, side="right"), len(cdf) - 1)
    q = cdf[i] - np.where(i > 0, cdf[np.maximum(i - 1, 0)], U64(0))
    with np.errstate(all="ignore"):
        inv_p = (np.full(len(i), S, U64).astype(F32) / q.astype(F32)).astype(F32)
    return i.astype(U32), inv_p


def sample32_inv_p(O, v0, v1, v2, x, nf, u_a, u_b, inv_p):
    """nee_scenes.sample32 with inv_p where it takes float(L): (wd [n, 3], g [n], valid [n]); the light's unit normal as its
    shade record's"""
    with np.errstate(all="ignore"):
        e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
        cr = N.cross(O, e1, e2)
        nl = normalize(O, cr)
        su = np.sqrt(u_a).astype(F32)
        b0 = (F32(1.0) - su).astype(F32)
        b1 = (su * (F32(1.0) - u_b).astype(F32)).astype(F32)
        b2 = (su * u_b).astype(F32)
        y = fma(O, v2, b2[:, None], fma(O, v1, b1[:, None], (v0 * b0[:, None]).astype(F32)))
        w = (y - x).astype(F32)
        r2 = dot(O, w, w)
        wd = normalize(O, w)
        cs = dot(O, nf, wd)
        cl = np.abs(dot(O, nl, wd))
        a2 = np.sqrt(dot(O, cr, cr)).astype(F32)
        valid = (cs > 0) & (cl > 0) & (r2 > 0) & (a2 > 0)
        g = (((cs * cl).astype(F32) * (a2 * np.asarray(inv_p, F32)).astype(F32)).astype(F32) / (N.K2PI * r2).astype(F32)).astype(F32)
    return wd, g, valid


# ------------------------------------------------------------------------------------------ weights for the table's tests
def skewed_weights(n, seed=47):
    """n seeded weights over eleven decades, a few of them 0"""
    g = np.random.default_rng(seed + n)
    w = (10.0 ** g.uniform(-8, 3, n)).astype(F32)
    w[g.random(n) < 0.05] = 0
    if n > 2:
        w[g.integers(0, n)] = F32(4096.0)          # the maximum, somewhere
    return w


HOSTILE = ("zeros_between", "all_zero", "one_huge", "subnormals", "nan_inf", "equal", "ratio_below", "ratio_at")


def hostile_weights(n, kind):
    """n weights of one of the HOSTILE kinds: zeros between positives; all zeros; one weight of 1e30 beside ones; subnormals
    (beside a normal maximum and alone); NaN, infinities and negatives between positives; equal weights; a ratio to the maximum
    just below 2^-16 (quantises to 0, lifted to 1) and exactly 2^-16 (quantises to 1)"""
    g = np.random.default_rng(53 + n)
    one = np.ones(n, F32)
    if kind == "zeros_between":
        w = one.copy()
        w[g.random(n) < 0.5] = 0
        w[::7] = 0
        return w
    if kind == "all_zero":
        return np.zeros(n, F32)
    if kind == "one_huge":
        w = one.copy()
        w[n // 2] = F32(1e30)
        return w
    if kind == "subnormals":
        w = np.full(n, 3, U32).view(F32).copy()     # 3 * 2^-149
        w[1::2] = np.full(len(w[1::2]), 0x00400000, U32).view(F32)
        if n > 4:
            w[n // 3] = F32(2.0) ** -120
        return w
    if kind == "nan_inf":
        w = (one * F32(0.5)).copy()
        w[0::5] = np.nan
        w[1::5] = np.inf
        w[2::5] = -np.inf
        w[3::5] = F32(-1.0)
        return w
    if kind == "equal":
        return np.full(n, F32(0.3), F32)
    if kind == "ratio_below":
        w = np.full(n, np.nextafter(F32(2.0) ** -16, F32(0)), F32)
        w[n - 1] = 1
        return w
    if kind == "ratio_at":
        w = np.full(n, F32(2.0) ** -16, F32)
        w[0] = 1
        return w
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------ scenes
RECEIVER_QUAD = [(-2.3, -1.8, 0.0), (2.3, -1.8, 0.0), (2.3, 1.8, 0.0), (-2.3, 1.8, 0.0)]
DIM_KE = (0.5, 0.25, 1.0)                          # the trapezoid of unequal_lamps: an eighth of nee_scenes.RECEIVER_KE
SQUARE_A = np.array([(1.0, 0.5, 2.0), (2.0, 0.5, 2.0), (2.0, 1.5, 2.0), (1.0, 1.5, 2.0)], np.float64)
SQUARE_B = np.array([(-2.0, -1.5, 1.5), (-1.0, -1.5, 1.5), (-1.0, -0.5, 1.5), (-2.0, -0.5, 1.5)], np.float64)
SECOND_LAMP = np.array([(0.5, 0.75, -2.0), (0.75, 0.75, -2.0), (0.75, 0.75, -1.75), (0.5, 0.75, -1.75)], np.float64)
SECOND_LAMP_KE = (8.0, 6.0, 2.0)


def unequal_lamps():
    """the receiver under two lamps of unequal Ke: nee_paths.two_lamps' quads without its degenerate triangle, the large trapezoid
    dim and the small quad bright.  Materials: 0 the receiver, 1 the trapezoid, 2 the small lamp"""
    quads = np.array([RECEIVER_QUAD, N.RECEIVER_LAMP, NP.SMALL_LAMP], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1, 2]))
    materials = P._materials((N.RECEIVER_KD,), (DIM_KE, NP.SMALL_LAMP_KE))
    return P.Scene("nee_unequal_lamps", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)


def equal_lamps():
    """the receiver under two unit squares of dyadic corners and one Ke: four emissive triangles of equal weight, bit for bit
    (every cross product is exact), so the table holds 65536, 131072, ... and L = 4 divides 2^16: the weighted pick names
    floor(m L / 2^24), which is the uniform pick's entry because u_l * 4 is exact, and inv_p = 4.0f = float(L)"""
    quads = np.array([RECEIVER_QUAD, SQUARE_A, SQUARE_B], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1, 1]))
    materials = P._materials((N.RECEIVER_KD,), (N.RECEIVER_KE,))
    return P.Scene("nee_equal_lamps", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)


def glass_room_two_lamps(form="small"):
    """dielectric_scenes.glass_room with a second, smaller and brighter lamp under its ceiling: (scene, glass, records)"""
    import dielectric_scenes as DS
    scene, glass = DS.glass_room(form)
    extra, _ = P._with_form(form if form != "odd" else "small", np.array([SECOND_LAMP], np.float64), np.array([0]))
    n_mat = len(scene.materials)
    tris = P._frozen(np.concatenate([np.asarray(scene.tris, F32).reshape(-1, 9), np.asarray(extra, F32).reshape(-1, 9)]))
    mat = P._frozen(np.concatenate([np.asarray(scene.tri_material), np.full(len(extra), n_mat)]).astype(np.uint32), np.uint32)
    materials = P._frozen(np.concatenate([np.asarray(scene.materials, F32), F32([(0.5, 0.5, 0.5) + SECOND_LAMP_KE])]))
    scene = scene._replace(name="glass_room_two_lamps", tris=tris, tri_material=mat, materials=materials)
    return scene, glass, DS.records(scene, None, glass)
