"""The weighted light pick of next-event estimation (RTPT_FLAG_EXT_NEE_POWER; csrc/light_sample.hpp states the rules,
csrc/light_table.hip builds the table) restated in numpy for test_nee_power_*.py: the weights, the cumulative table, the pick,
the sample that takes the inverse of the pick's probability, and a path walker.

Everything the device fixes is integer arithmetic or one correctly rounded float32 operation at a time, so numpy gives the same
bits: weights() is sample32's a2 times the largest |Ke| channel, table() the maximum, the quantisation and the integer running
sum, pick_power() the draw's 24 bits scaled into [0, S) and a binary search (numpy's searchsorted, side="right": the smallest i
with C_i > t).  walk_nee_power is nee_sphere.walk_nee_sphere's loop with the weighted pick and inv_p where `power`, and with
nee_paths.walk_nee's textures; with `power` off it takes the uniform pick and is that walker, which test_nee_power_cpu.py asks
for bit by bit."""
import numpy as np

import contract_cases as CC
import nee_paths as NP
import nee_scenes as N
import nee_sphere as NS
import pathtrace_scenes as P
from dielectric_scenes import _closest_hits, _contract, _primary, _rng_next, dot, fma, interface32, normalize
from gbuffer_scenes import fill_push_constants

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


# ------------------------------------------------------------------------------------------ the walker
def walk_nee_power(O, scene, W, H, segments, rec, lights, sphere=False, power=True, frame=0, rows=None, spp=1, texture=None):
    """nee_sphere.walk_nee_sphere with the weighted pick where `power` (and the list has entries), and nee_paths.walk_nee's
    `texture`: dict of IMAGE [H, W, 4], HIT_ID [H, W], rays, the walkers' counts, and picks: how often each entry of the list was
    drawn (int64 [L])"""
    cfg = P.configure(O.config_default(W, H), scene, segments, spp)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(scene), frame)
    y0, y1 = rows or (0, H)
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(W), indexing="ij")
    xs, ys = xs.ravel().astype(U32), ys.ravel().astype(U32)
    k = len(xs)
    seeds = np.stack([xs, ys, np.full(k, pc.frameNumber, U32), np.full(k, pc.sample_batch, U32)], 1)
    rng = O.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds, U32))[:, 0].copy()          # :297
    total, first_id = np.zeros((k, 3), F32), None
    lights = np.ascontiguousarray(lights, U32)
    count = dict(rays=0, samples=0, queries=0, lit=0, kept=0, dropped=0, sphere_samples=0, sphere_taken=0, sphere_valid=0,
                 sphere_dropped=0, sphere_kept=0, picks=np.zeros(len(lights), np.int64))
    rec = np.ascontiguousarray(rec, F32)
    cdf = table(weights(O, scene.tris, rec, lights)) if power and len(lights) else None
    for _ in range(spp):
        rng, d = _primary(O, cfg, rng, xs, ys)
        value, rng, ids = _path(O, cfg, pc, scene, rec, lights, cdf, bool(sphere), rng, d, count, texture)
        total = (total + value).astype(F32)                                                                  # :325
        first_id = ids if first_id is None else first_id
    image = np.zeros((H, W, 4), F32)
    hit_id = np.zeros((H, W), U32)
    image[y0:y1, :, :3] = (total / F32(spp)).astype(F32).reshape(y1 - y0, W, 3)                              # :328
    hit_id[y0:y1] = first_id.reshape(y1 - y0, W)
    return dict(IMAGE=image, HIT_ID=hit_id, **count)


def _path(O, cfg, pc, scene, rec, lights, cdf, sphere, rng, d, count, texture):
    """nee_sphere._path, statement for statement, but for the pick (cdf: the cumulative table, None: the uniform pick), the
    sample's weight and the texel"""
    tris = np.ascontiguousarray(scene.tris, F32)
    n_base, segments, k, L = len(rec), int(cfg.max_segments), len(d), len(lights)
    rng = rng.copy()
    light_c = F32(list(pc.lightPos))
    light_col = (F32(list(pc.currentCameraColor)) * F32(cfg.light_intensity)).astype(F32)                   # :281
    light_first = (light_col / F32(cfg.first_hit_light_divisor)).astype(F32)                                 # :229
    radius, ray_offset, tmax = F32(cfg.light_radius), F32(cfg.ray_offset), float(cfg.ray_tmax)
    r2 = NS.r2_of(radius)
    o = np.broadcast_to(F32(scene.cam), (k, 3)).astype(F32).copy()
    d = d.copy()
    acc = np.ones((k, 3), F32)
    radiance = np.zeros((k, 3), F32)                  # R: restarts at 0 with every sample
    sampled = np.zeros(k, bool)                       # the sampled bit (emissive triangles)
    sbit = np.zeros(k, bool)                          # the sphere bit: the primary ray starts with both clear
    alive = np.ones(k, bool)
    first_id = np.zeros(k, U32)
    for seg in range(segments):
        idx = np.flatnonzero(alive)
        if not len(idx):
            break
        oo, dd = o[idx], d[idx]
        ids, b1, b2 = _closest_hits(O, tris, oo, dd, tmax)
        count["rays"] += len(idx)
        if seg == 0:
            first_id[idx] = ids
        lit = O.contract_array(CC.fn_index("ray_hits_light"), np.ascontiguousarray(np.concatenate(
            [oo, dd, np.broadcast_to(light_c, oo.shape), np.full((len(idx), 1), radius, F32)], 1), F32).view(U32))[:, 0] != 0
        acc[idx[lit]] = (acc[idx[lit]] * (light_first if seg == 0 else light_col)).astype(F32)       # :229, :233
        acc[idx[lit][sbit[idx[lit]]]] = 0             # the hit before sampled the sphere: this hit's light is counted there
        if seg > 0:
            count["sphere_dropped"] += int(sbit[idx[lit]].sum())
            count["sphere_kept"] += int((~sbit[idx[lit]]).sum())
        sky = ~lit & (ids == 0)
        acc[idx[sky]] = (acc[idx[sky]] * _contract(O, "sky_color", dd[sky])).astype(F32)             # :266
        alive[idx[lit | sky]] = False
        hit = ~lit & (ids != 0)
        m = rec[(ids[hit].astype(np.int64) - 1) % n_base]
        emissive = m[:, 7] != 0
        j = idx[hit]
        acc[j[emissive]] = (acc[j[emissive]] * m[emissive, 4:7]).astype(F32)
        acc[j[emissive][sampled[j[emissive]]]] = 0    # the hit before sampled the lights: this emission is counted there
        if seg > 0:
            count["dropped"] += int(sampled[j[emissive]].sum())
            count["kept"] += int((~sampled[j[emissive]]).sum())
        alive[j[emissive]] = False
        keep = ~emissive
        j, m = j[keep], m[keep]
        b1, b2, dd = b1[hit][keep], b2[hit][keep], dd[hit][keep]
        b0 = ((F32(1.0) - b1).astype(F32) - b2).astype(F32)                                          # :134
        alb = m[:, 0:3]
        if texture is not None:
            alb = (alb * NP._texels(O, texture, (ids[hit][keep].astype(np.int64) - 1) % n_base, b0, b1, b2)).astype(F32)
        acc[j] = (acc[j] * alb).astype(F32)                                                          # :244
        if seg + 1 >= segments:                       # the last segment: no light draw, no shadow query; the bounce's two draws
            rng[j] = _rng_next(O, _rng_next(O, rng[j])[0])[0]      # only move the stream (:256-257)
            break
        tri = tris[ids[hit][keep].astype(np.int64) - 1]
        pos = fma(O, tri[:, 6:9], b2[:, None], fma(O, tri[:, 3:6], b1[:, None], (tri[:, 0:3] * b0[:, None]).astype(F32)))   # :137
        e1, e2 = (tri[:, 3:6] - tri[:, 0:3]).astype(F32), (tri[:, 6:9] - tri[:, 0:3]).astype(F32)
        n = normalize(O, _contract(O, "cross", e1, e2))                                              # :150
        w = m[:, 3]
        glass = w > 0
        mirror = ~glass & (w.view(U32) != 0)
        diffuse = ~glass & ~mirror
        nf = np.where((dot(O, n, dd) < 0)[:, None], n, -n).astype(F32)                               # :247
        q = np.flatnonzero(diffuse)
        jq = j[q]
        x = fma(O, ray_offset, nf[q], pos[q])                                                         # :250, the bounce's origin
        tri_gain = None
        if L:                                         # ---- the triangle sample: three draws, its gain added behind the sphere's
            r, u_l = _rng_next(O, rng[jq])
            r, u_a = _rng_next(O, r)
            r, u_b = _rng_next(O, r)
            rng[jq] = r
            if cdf is not None:                       # the weighted pick, and the inverse of its probability in the weight
                entry, inv_p = pick_power(cdf, u_l)
                id1 = lights[entry]
                lt = tris[id1.astype(np.int64) - 1]
                wd, g, valid = sample32_inv_p(O, lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, nf[q], u_a, u_b, inv_p)
            else:
                entry = N.pick(u_l, np.full(len(q), L))
                id1 = lights[entry]
                lt = tris[id1.astype(np.int64) - 1]
                s = N.sample32(O, N.cases_of(lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, nf[q], u_l, u_a, u_b, L))[:, :8].view(F32)
                wd, g, valid = s[:, 3:6], s[:, 6], s[:, 7] != 0
            count["picks"] += np.bincount(entry, minlength=L)
            ke = rec[(id1.astype(np.int64) - 1) % n_base, 4:7]
            gain = (((acc[jq] * ke).astype(F32)) * g[:, None]).astype(F32)                            # (T * Ke) * g
            seen, _, _ = _closest_hits(O, tris, x[valid], wd[valid], tmax)
            reached = seen == id1[valid]
            tri_gain = (jq[valid][reached], gain[valid][reached])
            count["rays"] += int(valid.sum())
            count["samples"] += len(q)
            count["queries"] += int(valid.sum())
            count["lit"] += int(reached.sum())
            sampled[jq] = True                        # valid or not
            sampled[j[~diffuse]] = False              # a specular or dielectric hit clears the bit
        if sphere:                                    # ---- the sphere sample: two draws, no query, into R first
            r, u_c = _rng_next(O, rng[jq])
            r, u_p = _rng_next(O, r)
            rng[jq] = r
            s = NS.sphere32(O, NS.cases_of(x, nf[q], light_c, r2, u_c, u_p)).view(F32)
            taken, valid = s[:, 4] != 0, s[:, 5] != 0
            gain = (((acc[jq] * light_col).astype(F32)) * s[:, 3:4]).astype(F32)                      # (T * light_col) * g
            radiance[jq[valid]] = (radiance[jq[valid]] + gain[valid]).astype(F32)
            count["sphere_samples"] += len(q)
            count["sphere_taken"] += int(taken.sum())
            count["sphere_valid"] += int(valid.sum())
            sbit[jq] = taken                          # set by a taken sample, valid or not; cleared by one not taken
            sbit[j[~diffuse]] = False                 # a specular or dielectric hit clears the bit
        if tri_gain is not None:
            radiance[tri_gain[0]] = (radiance[tri_gain[0]] + tri_gain[1]).astype(F32)
        rng_j, u1 = _rng_next(O, rng[j])                                                             # :256
        rng_j, u2 = _rng_next(O, rng_j)                                                              # :257
        rng[j] = rng_j
        off = np.full(len(j), ray_offset, F32)
        sn_cs = _contract(O, "sincos2pi", u1)
        sn, cs = sn_cs[:, 0], sn_cs[:, 1]
        u = fma(O, F32(2.0), u2, F32(-1.0))
        rho = np.sqrt(fma(O, -u, u, F32(1.0))).astype(F32)                                           # :258
        dn = normalize(O, np.stack([fma(O, rho, cs, nf[:, 0]), fma(O, rho, sn, nf[:, 1]), (nf[:, 2] + u).astype(F32)], 1))   # :259-261
        if mirror.any():                              # specular.hpp: the lobe around the mirror direction
            nm, dm, gl = nf[mirror], dd[mirror], np.abs(w[mirror])
            c2 = (F32(-2.0) * dot(O, nm, dm)).astype(F32)
            refl = fma(O, c2[:, None], nm, dm)
            sph = np.stack([(rho[mirror] * cs[mirror]).astype(F32), (rho[mirror] * sn[mirror]).astype(F32), u[mirror]], 1)
            lobe = normalize(O, fma(O, gl[:, None], sph, refl))
            dn[mirror] = lobe
            absorbed = ~(dot(O, nm, lobe) > 0)
            gone = j[mirror][absorbed]
            acc[gone] = 0
            alive[gone] = False
        if glass.any():                               # dielectric.hpp
            dg, transmitted, _, _ = interface32(O, n[glass], dd[glass], u1[glass], w[glass], m[glass, 4], m[glass, 5])
            dn[glass] = dg
            off[glass] = np.where(transmitted, -ray_offset, ray_offset)
        o[j] = fma(O, off[:, None], nf, pos)                                                          # :250
        d[j] = dn
    return (radiance + acc).astype(F32), rng, first_id                                                # R + terminal


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
