"""Multiple importance sampling of next-event estimation (RTPT_FLAG_EXT_NEE_MIS; csrc/light_sample.hpp states the rules) restated
in numpy for test_nee_mis_*.py: the two weights of the power heuristic, the light sample's weight function at a point a bounce
hit, the search for a hit emitter's entry of the light list, a path walker and the scene with a close emitter.

Everything the device fixes is one correctly rounded float32 operation at a time (numpy's products, sums and divisions, the
contract's dot, cross, normalize and fused multiply-add through dielectric_scenes) or integer arithmetic, so numpy gives the same
bits.  find() is the binary search of csrc/light_list_host.hpp, step for step on arrays of queries; test_nee_mis_cpu.py holds it to
np.searchsorted.  walk_nee_mis is nee_power.walk_nee_power's loop, restated here, with the three rules where `mis` (and the list
has entries): the sample's g becomes g * m(g), a diffuse hit that goes on records the cosine cb of its new direction, and an
emissive triangle met with the sampled bit set ends the path with (T * Ke) * wb(g_hit) instead of 0.  With `mis` off it is that
walker, which test_nee_mis_cpu.py asks for bit by bit.  `frames`: many frames of one scene walked as one batch of paths (a path's
stream depends on its pixel and its frame number only), for the estimator's tests."""
import numpy as np

import contract_cases as CC
import nee_paths as NP
import nee_power as PW
import nee_scenes as N
import nee_sphere as NS
import pathtrace_scenes as P
from dielectric_scenes import _closest_hits, _contract, _primary, _rng_next, dot, fma, interface32, normalize
from gbuffer_scenes import fill_push_constants

F32, U32, U64 = np.float32, np.uint32, np.uint64
ONE = F32(1.0)
INF = F32(np.inf)


# ------------------------------------------------------------------------------------------ the weights
def m_light(g):
    """m(g) = 1 / (1 + g * g), float32: the light side of the power heuristic"""
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        g2 = (g * g).astype(F32)
        return (ONE / (ONE + g2).astype(F32)).astype(F32)


def wb(g):
    """wb(g) = g2 / (1 + g2) where g2 = g * g < +inf, else 1 (a NaN fails the comparison), float32: the bounce side"""
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        g2 = (g * g).astype(F32)
        return np.where(g2 < INF, (g2 / (ONE + g2).astype(F32)).astype(F32), ONE).astype(F32)


def gm(g):
    """g * m(g): the light sample's weight, one multiply behind sample()'s division"""
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        return (g * m_light(g)).astype(F32)


def weights64(g):
    """(wb, gm) in float64 from the float32 g as it is"""
    g = np.asarray(g, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        g2 = g * g
        return g2 / (1 + g2), g / (1 + g2)


def g_hit(O, v0, v1, v2, o, d, b1, b2, cb, inv_p):
    """light::hit_weight, operation by operation: the light sample's weight function at the point with barycentrics (b1, b2) of
    the emitter (v0, v1, v2) that the ray (o, d) hit; the emitter's unit normal as its shade record's, b0 as hit_barycentrics"""
    v0, v1, v2, o, d = (np.asarray(a, F32).reshape(-1, 3) for a in (v0, v1, v2, o, d))
    b1, b2, cb, inv_p = (np.asarray(a, F32).ravel() for a in (b1, b2, cb, inv_p))
    with np.errstate(all="ignore"):
        b0 = ((ONE - b1).astype(F32) - b2).astype(F32)
        e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
        cr = N.cross(O, e1, e2)
        nl = normalize(O, cr)                                                                          # raytrace.comp.glsl:150
        y = fma(O, v2, b2[:, None], fma(O, v1, b1[:, None], (v0 * b0[:, None]).astype(F32)))           # bary_point
        w = (y - o).astype(F32)
        r2 = dot(O, w, w)
        cl = np.abs(dot(O, nl, d))
        a2 = np.sqrt(dot(O, cr, cr)).astype(F32)
        return (((cb * cl).astype(F32) * (a2 * inv_p).astype(F32)).astype(F32) / (N.K2PI * r2).astype(F32)).astype(F32)


def cases_of(v0, v1, v2, o, d, b1, b2, cb, inv_p):
    """[n, 20] float32 of rtpt_selftest_mis_weight's input (word 19 is not read: 0)"""
    n = len(np.asarray(o).reshape(-1, 3))
    f = np.concatenate([np.broadcast_to(np.asarray(a, F32), (n, 3)) for a in (v0, v1, v2, o, d)] +
                       [np.broadcast_to(np.asarray(a, F32), (n,))[:, None] for a in (b1, b2, cb, inv_p, 0.0)], 1).astype(F32)
    return np.ascontiguousarray(f)


def mis_weight32(O, cases):
    """[n, 3] float32 (g_hit, wb(g_hit), g_hit * m(g_hit)) of cases [n, 20]: what rtpt_selftest_mis_weight returns"""
    c = np.ascontiguousarray(cases, F32).reshape(-1, 20)
    g = g_hit(O, c[:, 0:3], c[:, 3:6], c[:, 6:9], c[:, 9:12], c[:, 12:15], c[:, 15], c[:, 16], c[:, 17], c[:, 18])
    return np.stack([g, wb(g), gm(g)], 1).astype(F32)


# ------------------------------------------------------------------------------------------ the search
def find(ids, queries):
    """uint32 [k]: rtpt_light::find of every query on the ascending list ids [n] — the index of the entry, n where the list does
    not hold the id.  The device's loop, step for step, on all queries at once; every index read lies in [0, n)"""
    ids = np.ascontiguousarray(ids, U32).ravel()
    q = np.ascontiguousarray(queries, U32).ravel()
    n = len(ids)
    lo, hi = np.zeros(len(q), np.int64), np.full(len(q), n, np.int64)
    while True:
        go = lo < hi
        if not go.any():
            break
        mid = lo + ((hi - lo) >> 1)
        assert n > 0 and mid[go].min() >= 0 and mid[go].max() < n
        less = np.zeros(len(q), bool)
        less[go] = ids[mid[go]] < q[go]
        lo = np.where(go & less, mid + 1, lo)
        hi = np.where(go & ~less, mid, hi)
    found = lo < n
    found[found] = ids[lo[found]] == q[found]
    return np.where(found, lo, n).astype(U32)


def hit_inv_p(lights, cdf, id1):
    """(reached bool [k], inv_p float32 [k]) for the emitters id1 [k] a bounce hit: float(L) for the uniform pick (cdf None); for
    the weighted pick float(S) / float(q_i) of the emitter's entry, not reached where q_i == 0 or the list does not hold the id"""
    L = len(lights)
    id1 = np.asarray(id1, U32).ravel()
    if cdf is None:
        return np.ones(len(id1), bool), np.full(len(id1), F32(L), F32)
    cdf = np.asarray(cdf, U64)
    i = find(lights, id1).astype(np.int64)
    held = i < L
    ic = np.minimum(i, L - 1)
    q = cdf[ic] - np.where(ic > 0, cdf[np.maximum(ic - 1, 0)], U64(0))
    reached = held & (q > 0)
    with np.errstate(all="ignore"):
        inv_p = (np.full(len(id1), cdf[-1], U64).astype(F32) / q.astype(F32)).astype(F32)
    return reached, np.where(reached, inv_p, F32(0)).astype(F32)


# ------------------------------------------------------------------------------------------ the walker
def walk_nee_mis(O, scene, W, H, segments, rec, lights, mis=True, power=False, sphere=False, frame=0, rows=None, spp=1, texture=None,
                 frames=None):
    """nee_power.walk_nee_power with RTPT_FLAG_EXT_NEE_MIS's rules where `mis` (and the list has entries): dict of IMAGE [H, W, 4],
    HIT_ID [H, W], rays, that walker's counts and picks, and
      weighted        emissive triangles met behind the first segment with the sampled bit set (the walker's `dropped`): with `mis`
                      they end the path with (T * Ke) * wb, without it with 0
      wb_min, wb_max  the smallest and the largest wb among them (with `mis`; 1, 0 where there was none)
    frames: a sequence of frame numbers walked as one batch; IMAGE is then [len(frames), H, W, 4], HIT_ID [len(frames), H, W], and
    `frame` is not read"""
    cfg = P.configure(O.config_default(W, H), scene, segments, spp)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(scene), frame)
    y0, y1 = rows or (0, H)
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(W), indexing="ij")
    xs, ys = xs.ravel().astype(U32), ys.ravel().astype(U32)
    per = len(xs)
    fr = np.asarray([pc.frameNumber] if frames is None else list(frames), U32)
    xs, ys, fn = np.tile(xs, len(fr)), np.tile(ys, len(fr)), np.repeat(fr, per)
    k = len(xs)
    seeds = np.stack([xs, ys, fn, np.full(k, pc.sample_batch, U32)], 1)
    rng = O.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds, U32))[:, 0].copy()          # :297
    total, first_id = np.zeros((k, 3), F32), None
    lights = np.ascontiguousarray(lights, U32)
    count = dict(rays=0, samples=0, queries=0, lit=0, kept=0, dropped=0, sphere_samples=0, sphere_taken=0, sphere_valid=0,
                 sphere_dropped=0, sphere_kept=0, picks=np.zeros(len(lights), np.int64), weighted=0, wb_min=1.0, wb_max=0.0)
    rec = np.ascontiguousarray(rec, F32)
    cdf = PW.table(PW.weights(O, scene.tris, rec, lights)) if power and len(lights) else None
    for _ in range(spp):
        rng, d = _primary(O, cfg, rng, xs, ys)
        value, rng, ids = _path(O, cfg, pc, scene, rec, lights, cdf, bool(sphere), bool(mis) and len(lights) > 0, rng, d, count, texture)
        total = (total + value).astype(F32)                                                                  # :325
        first_id = ids if first_id is None else first_id
    image = np.zeros((len(fr), H, W, 4), F32)
    hit_id = np.zeros((len(fr), H, W), U32)
    image[:, y0:y1, :, :3] = (total / F32(spp)).astype(F32).reshape(len(fr), y1 - y0, W, 3)                 # :328
    hit_id[:, y0:y1] = first_id.reshape(len(fr), y1 - y0, W)
    if frames is None:
        image, hit_id = image[0], hit_id[0]
    return dict(IMAGE=image, HIT_ID=hit_id, **count)


def _path(O, cfg, pc, scene, rec, lights, cdf, sphere, mis, rng, d, count, texture):
    """nee_power._path, statement for statement, but for the three rules of `mis` (marked MIS)"""
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
    cb = np.zeros(k, F32)                             # MIS: the cosine of the last diffuse bounce; read only where `sampled`
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
        again = sampled[j[emissive]]                  # the hit before sampled the lights
        if mis:                                       # MIS: this emission is one of two estimators, (T * Ke) * wb(g_hit)
            je = j[emissive][again]
            if len(je):
                eid = ids[hit][emissive][again]
                et = tris[eid.astype(np.int64) - 1]
                reached, inv_p = hit_inv_p(lights, cdf, eid)
                gh = g_hit(O, et[:, 0:3], et[:, 3:6], et[:, 6:9], oo[hit][emissive][again], dd[hit][emissive][again],
                           b1[hit][emissive][again], b2[hit][emissive][again], cb[je], inv_p)
                w_b = np.where(reached, wb(gh), ONE).astype(F32)
                acc[je] = (acc[je] * w_b[:, None]).astype(F32)
                count["wb_min"] = min(count["wb_min"], float(w_b.min()))
                count["wb_max"] = max(count["wb_max"], float(w_b.max()))
        else:
            acc[j[emissive][again]] = 0               # ... this emission is counted there
        if seg > 0:
            count["dropped"] += int(again.sum())
            count["weighted"] += int(again.sum())
            count["kept"] += int((~again).sum())
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
                entry, inv_p = PW.pick_power(cdf, u_l)
                id1 = lights[entry]
                lt = tris[id1.astype(np.int64) - 1]
                wd, g, valid = PW.sample32_inv_p(O, lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, nf[q], u_a, u_b, inv_p)
            else:
                entry = N.pick(u_l, np.full(len(q), L))
                id1 = lights[entry]
                lt = tris[id1.astype(np.int64) - 1]
                s = N.sample32(O, N.cases_of(lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, nf[q], u_l, u_a, u_b, L))[:, :8].view(F32)
                wd, g, valid = s[:, 3:6], s[:, 6], s[:, 7] != 0
            if mis:                                   # MIS: gm = g * m(g), one multiply behind the division
                g = gm(g)
            count["picks"] += np.bincount(entry, minlength=L)
            ke = rec[(id1.astype(np.int64) - 1) % n_base, 4:7]
            with np.errstate(all="ignore"):
                gain = (((acc[jq] * ke).astype(F32)) * g[:, None]).astype(F32)                        # (T * Ke) * g
            seen, _, _ = _closest_hits(O, tris, x[valid], wd[valid], tmax)
            reached = seen == id1[valid]
            tri_gain = (jq[valid][reached], gain[valid][reached])
            count["rays"] += int(valid.sum())
            count["samples"] += len(q)
            count["queries"] += int(valid.sum())
            count["lit"] += int(reached.sum())
            sampled[jq] = True                        # valid or not
            sampled[j[~diffuse]] = False              # a specular or dielectric hit clears the bit
        if sphere:                                    # ---- the sphere sample: two draws, no query, into R first; never weighed
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
        if mis:                                       # MIS: the cosine the diffuse bounce leaves with, behind the normalize
            cb[jq] = dot(O, nf[q], dn[q])
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


# ------------------------------------------------------------------------------------------ operands
G_HOSTILE = np.array([0.0, 1e-45, 1e-40, 1.17549435e-38, 1e-20, 0.5, 1.0, 2.0, 2.0 ** 63, 2.0 ** 64, 2.0 ** 64 * 1.5, 1e30, 3.4028235e38,
                      np.inf, np.nan, -1.0, -np.inf], np.float64).astype(F32)
G_HOSTILE.setflags(write=False)


def seeded_g(n=4096, seed=67):
    """n weights over twelve decades around 1, log-uniform"""
    g = (10.0 ** np.random.default_rng(seed).uniform(-6, 6, n)).astype(F32)
    g.setflags(write=False)
    return g


def seeded_cases(n=4096, seed=71):
    """[n, 20]: emitters of random vertices in [-1, 1]^3, a hit point of random barycentrics on each, the ray's origin at a distance
    log-uniform in [0.01, 4] along a random direction, cb uniform in (0, 1], inv_p log-uniform in [1, 2^20]"""
    r = np.random.default_rng(seed)
    v = r.uniform(-1, 1, (n, 3, 3)).astype(F32)
    su, ub = np.sqrt(r.random(n)), r.random(n)
    b1, b2 = (su * (1 - ub)).astype(F32), (su * ub).astype(F32)
    y = v[:, 0] * (1 - b1 - b2)[:, None] + v[:, 1] * b1[:, None] + v[:, 2] * b2[:, None]
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = 10.0 ** r.uniform(-2, np.log10(4.0), n)
    o = y - dist[:, None] * d
    out = cases_of(v[:, 0], v[:, 1], v[:, 2], o, d, b1, b2, 1.0 - r.random(n), 2.0 ** r.uniform(0, 20, n))
    out.setflags(write=False)
    return out


def hostile_cases():
    """[n, 20]: on one emitter — cl = 0 (the ray in the emitter's plane), cb = 0, inv_p = inf (q_i = 0 by the formula) with cb * cl
    positive and zero, inv_p = NaN and 0, r2 = 0 (the origin on the hit point), r2 subnormal, a degenerate emitter (a2 = 0), huge
    and tiny operands (g2 overflows, g underflows), cb negative and NaN, barycentrics outside the triangle"""
    v0, v1, v2 = F32([0, 0, 0]), F32([1, 0, 0]), F32([0, 0, 1])                       # in the plane y = 0, normal (0, -1, 0)
    down, o = F32([0, -1, 0]), F32([0.25, 1, 0.25])
    rows = [
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, 2.0),                            # an ordinary hit
        cases_of(v0, v1, v2, F32([-1, 0, 0.25]), F32([1, 0, 0]), 0.25, 0.25, 0.5, 2.0),  # cl = 0
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.0, 2.0),                            # cb = 0
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, np.inf),                         # q_i = 0: inv_p = inf
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.0, np.inf),                         # ... times 0: NaN
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, np.nan),
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, 0.0),
        cases_of(v0, v1, v2, F32([0.25, 0, 0.25]), down, 0.25, 0.25, 0.5, 2.0),         # r2 = 0
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** -70, 0.25]), down, 0.25, 0.25, 0.5, 2.0),  # r2 = 2^-140
        cases_of(v0, v1, v1, o, down, 0.25, 0.25, 0.5, 2.0),                            # a2 = 0
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** -20, 0.25]), down, 0.25, 0.25, 1.0, 2.0 ** 30),   # g2 overflows
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** -40, 0.25]), down, 0.25, 0.25, 1.0, 2.0 ** 60),   # g overflows
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** 40, 0.25]), down, 0.25, 0.25, 2.0 ** -40, 1.0),   # g underflows
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, -0.5, 2.0),                           # cb < 0 (no bounce leaves with one)
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, np.nan, 2.0),
        cases_of(v0, v1, v2, o, down, 3.0, -2.5, 0.5, 2.0),                             # barycentrics outside
        cases_of(v0 * F32(1e18), v1 * F32(1e18), v2 * F32(1e18), o, down, 0.25, 0.25, 0.5, 2.0),   # the cross product overflows
    ]
    out = np.concatenate(rows)
    out.setflags(write=False)
    return out


FIND_SIZES = (1, 2, 3, 1000, (1 << 20) + 1025)


def find_case(n, seed=73):
    """(ids [n] ascending with gaps of 1 to 5 between neighbours, queries): both ends, every entry and every gap (of a list up to
    1,000 entries; of a longer one 4,096 seeded places), ids below, above and between the entries"""
    r = np.random.default_rng(seed + n)
    ids = (2 + np.cumsum(r.integers(1, 6, n))).astype(U32)
    at = np.arange(n) if n <= 1000 else np.unique(np.concatenate([[0, n - 1], r.integers(0, n, 4096)]))
    e = ids[at].astype(np.int64)
    q = np.concatenate([e, e + 1, e - 1, e + 2, [0, 1, 2, int(ids[0]) - 1, int(ids[-1]) + 1, 2 ** 32 - 1, 2 ** 31]])
    return ids, np.clip(q, 0, 2 ** 32 - 1).astype(U32)


# ------------------------------------------------------------------------------------------ scenes
WALL_LAMP = np.array([(-2.2, 1.6, 0.02), (2.2, 1.6, 0.02), (2.2, 1.6, 1.0), (-2.2, 1.6, 1.0)], np.float64)


def wall_lamp():
    """nee_power's receiver quad with an emissive wall standing on it, just outside the view of nee_scenes.receiver()'s camera: the
    hit points next to the wall are where the area sample's weight is unbounded.  Materials: 0 the receiver, 1 the wall"""
    quads = np.array([PW.RECEIVER_QUAD, WALL_LAMP], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1]))
    materials = P._materials((N.RECEIVER_KD,), (N.RECEIVER_KE,))
    return P.Scene("nee_wall_lamp", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)
