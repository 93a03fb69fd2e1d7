"""The sphere sample of next-event estimation (RTPT_FLAG_EXT_NEE_SPHERE; csrc/light_sample.hpp states the rules and the
arithmetic) for test_nee_sphere_*.py: its numpy restatements, a path walker and the scenes.

sphere32 follows light::sphere_sample one float32 operation per device operation, through the pieces of dielectric_scenes (the
contract's dot, normalize, sincos2pi and fused multiply-add; numpy's square root, products and divisions, all correctly rounded):
it is what tests/test_nee_sphere_gpu.py holds the device function to, bit for bit.  sphere64 is the same in float64 from the
float32 operands as they are, the same orthonormal pair included (the direction depends on it).

walk_nee_sphere is the loop of nee_paths._path_nee plus the sphere's rules: two draws behind the triangle sample's three, the
sphere's gain into R before the triangle's, the sphere bit beside the sampled bit.  With sphere=False it takes no draw of its own
and is nee_paths.walk_nee (with an empty list: dielectric_scenes.walk), which tests/test_nee_sphere_cpu.py asks for bit by bit
before anything else is concluded from it.  A scene without a material table walks with normal_keyed_records."""
from functools import lru_cache

import numpy as np

import contract_cases as CC
import dielectric_scenes as DS
import nee_paths as NP
import nee_scenes as N
import pathtrace_scenes as P
from dielectric_scenes import _closest_hits, _contract, _primary, _rng_next, dot, fma, interface32, normalize
from gbuffer_scenes import fill_push_constants

F32, U32 = np.float32, np.uint32
RADIUS = 0.2


# ------------------------------------------------------------------------------------------ the sample in float32 and float64
def cases_of(x, nf, c, r2, u_c, u_p):
    """[n, 12] uint32 words of rtpt_selftest_sphere_sample's input"""
    n = len(np.asarray(x).reshape(-1, 3))
    f = np.concatenate([np.broadcast_to(np.asarray(a, F32), (n, 3)) for a in (x, nf, c)] +
                       [np.broadcast_to(np.asarray(a, F32), (n,))[:, None] for a in (r2, u_c, u_p)], 1).astype(F32)
    return np.ascontiguousarray(f.view(U32))


def sphere32(O, cases):
    """[n, 6] uint32 words (wd, g, taken and valid as 1.0 / 0.0; wd and g 0 where not taken) of cases [n, 12]:
    light::sphere_sample, operation by operation"""
    f = np.ascontiguousarray(cases, U32).reshape(-1, 12).view(F32)
    x, nf, c, r2, u_c, u_p = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9], f[:, 10], f[:, 11]
    one = F32(1.0)
    with np.errstate(all="ignore"):
        dc = (c - x).astype(F32)
        d2 = dot(O, dc, dc)
        w = normalize(O, dc)
        q = (r2 / d2).astype(F32)
        cm = np.sqrt((one - q).astype(F32)).astype(F32)
        k = (q / (one + cm).astype(F32)).astype(F32)
        ct = fma(O, -u_c, k, one)
        v = fma(O, -ct, ct, one)
        st = np.sqrt(np.where(F32(0.0) < v, v, F32(0.0)).astype(F32)).astype(F32)          # glsl_max(0, v): 0 where v is NaN
        sc = _contract(O, "sincos2pi", u_p)
        sp, cp = sc[:, 0], sc[:, 1]
        wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
        sg = np.copysign(one, wz).astype(F32)
        a = (F32(-1.0) / (sg + wz).astype(F32)).astype(F32)
        b_ = ((wx * wy).astype(F32) * a).astype(F32)
        sx = (sg * wx).astype(F32)
        t = np.stack([fma(O, sx, (wx * a).astype(F32), one), (sg * b_).astype(F32), -sx], 1)
        b = np.stack([b_, fma(O, wy, (wy * a).astype(F32), sg), -wy], 1)
        ac, as_ = (st * cp).astype(F32), (st * sp).astype(F32)
        wd = normalize(O, fma(O, ct[:, None], w, fma(O, as_[:, None], b, (ac[:, None] * t).astype(F32))))
        cs = dot(O, nf, wd)
        taken = d2 > r2
        valid = taken & (cs > 0)
        g = ((F32(2.0) * cs).astype(F32) * k).astype(F32)
    out = np.concatenate([wd, g[:, None], taken[:, None].astype(F32), valid[:, None].astype(F32)], 1).astype(F32).view(U32).copy()
    out[~taken, :4] = 0
    return np.ascontiguousarray(out)


def sphere64(cases):
    """the same in float64 from the float32 operands: dict of wd, g, taken, valid, cs, q, cw = dot(nf, w)"""
    f = np.ascontiguousarray(cases, U32).reshape(-1, 12).view(F32).astype(np.float64)
    x, nf, c, r2, u_c, u_p = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9], f[:, 10], f[:, 11]
    with np.errstate(all="ignore"):
        dc = c - x
        d2 = (dc * dc).sum(1)
        w = dc / np.sqrt(d2)[:, None]
        q = r2 / d2
        cm = np.sqrt(1 - q)
        k = q / (1 + cm)
        ct = 1 - u_c * k
        st = np.sqrt(np.maximum(0.0, 1 - ct * ct))
        sp, cp = np.sin(2 * np.pi * u_p), np.cos(2 * np.pi * u_p)
        wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
        sg = np.copysign(1.0, wz)
        a = -1.0 / (sg + wz)
        b_ = wx * wy * a
        t = np.stack([1 + sg * wx * wx * a, sg * b_, -sg * wx], 1)
        b = np.stack([b_, sg + wy * wy * a, -wy], 1)
        v = (st * cp)[:, None] * t + (st * sp)[:, None] * b + ct[:, None] * w
        wd = v / np.linalg.norm(v, axis=1, keepdims=True)
        cs = (nf * wd).sum(1)
        taken = d2 > r2
    return dict(wd=wd, g=2 * cs * k, taken=taken, valid=taken & (cs > 0), cs=cs, q=q, cw=(nf * w).sum(1))


def _draw(k):
    return (np.asarray(k, np.float64) * 2.0 ** -24).astype(F32)


def r2_of(radius):
    """PathtraceArgs::light_r2 = radius * radius in binary32"""
    return (F32(radius) * F32(radius)).astype(F32)


# ------------------------------------------------------------------------------------------ operands
@lru_cache(maxsize=None)
def seeded_cases(n=4096, seed=43):
    """the direction to the light uniform on the sphere, its distance uniform in [0.25, 4], radius 0.2, the faced normal uniform in
    solid angle within 60 degrees of that direction (the cosine of the tilt uniform in [1/2, 1]), the centre uniform in [-1, 1]^3,
    draws as exact::rng_next returns them: [n, 12] words"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(n, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    dist = rng.uniform(0.25, 4.0, n)
    c = rng.uniform(-1, 1, (n, 3))
    x = c - dist[:, None] * w
    ct = rng.uniform(0.5, 1.0, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    st = np.sqrt(1 - ct * ct)
    ref = np.where(np.abs(w[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = np.cross(w, ref)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(w, t)
    nf = (st * np.cos(ph))[:, None] * t + (st * np.sin(ph))[:, None] * b + ct[:, None] * w
    u = _draw(rng.integers(0, 2 ** 24, (n, 2)))
    out = cases_of(x, nf, c, r2_of(RADIUS), u[:, 0], u[:, 1])
    out.setflags(write=False)
    return out


HOSTILE = ("centre", "on", "on_minus", "on_plus", "inside", "w_plus_z", "w_minus_z", "w_z_minus_zero", "u_c_0", "u_c_top", "u_p_0",
           "u_p_top", "perpendicular", "light_far", "tiny", "huge", "q_subnormal")


@lru_cache(maxsize=None)
def hostile_cases():
    """one row per name of HOSTILE: x at the centre; d2 == r2 and r2 one ulp to either side; x inside; w = (0, 0, +-1) and w.z = -0;
    u_c at 0 and at 1 - 2^-24; u_p at 0 and next to 1; nf perpendicular to w; pathtrace_scenes.LIGHT_FAR; the radii of
    pathtrace_scenes.PLACEMENTS (0.2 x 10^-3 and 0.2 x 10^3, at the distances those scenes have); q subnormal"""
    r2 = r2_of(RADIUS)
    up, o = F32([0, 0, 1]), F32([0, 0, 0])
    top = _draw(2 ** 24 - 1)
    on = F32([0, 0, -RADIUS])                    # d2 = fma(0, 0, fma(0, 0, 0.2f * 0.2f)) = r2
    rows = {
        "centre": cases_of(o, up, o, r2, 0.5, 0.25),
        "on": cases_of(on, up, o, r2, 0.5, 0.25),
        "on_minus": cases_of(on, up, o, np.nextafter(r2, F32(0)), 0.5, 0.25),
        "on_plus": cases_of(on, up, o, np.nextafter(r2, F32(1)), 0.5, 0.25),
        "inside": cases_of(F32([0.05, 0, -0.1]), up, o, r2, 0.5, 0.25),
        "w_plus_z": cases_of(F32([0, 0, -1]), up, o, r2, 0.5, 0.25),
        "w_minus_z": cases_of(F32([0, 0, 1]), -up, o, r2, 0.5, 0.25),
        "w_z_minus_zero": cases_of(o, F32([1, 0, 0]), F32([1, 0, -0.0]), r2, 0.5, 0.25),
        "u_c_0": cases_of(F32([0.3, -0.4, -1]), up, o, r2, 0.0, 0.25),
        "u_c_top": cases_of(F32([0.3, -0.4, -1]), up, o, r2, top, 0.25),
        "u_p_0": cases_of(F32([0.3, -0.4, -1]), up, o, r2, 0.5, 0.0),
        "u_p_top": cases_of(F32([0.3, -0.4, -1]), up, o, r2, 0.5, top),
        "perpendicular": cases_of(F32([0, 0, -1]), F32([1, 0, 0]), o, r2, 0.5, 0.25),
        "light_far": cases_of(F32([0.1, -0.05, 0.5]), F32([0, 1, 0]), F32(P.LIGHT_FAR), r2, 0.5, 0.25),
        "tiny": cases_of(F32([3e-4, -4e-4, -1e-3]), up, o, r2_of(F32(RADIUS * 1e-3)), 0.5, 0.25),
        "huge": cases_of(F32([300, -400, -1000]), up, o, r2_of(F32(RADIUS * 1e3)), 0.5, 0.25),
        "q_subnormal": cases_of(F32([0, 0, -1e5]), up, o, F32(1e-30), 0.5, 0.25),
    }
    out = np.concatenate([rows[k] for k in HOSTILE])
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ records without a material table
def normal_keyed_records(O, scene):
    """[t, 8] float32: one diffuse record per triangle with the reference's normal-keyed colour (raytrace.comp.glsl:155-163) of its
    stored normal, nothing emissive — what shade_segment takes for a scene without a material table"""
    n = DS.stored_normals(O, scene.tris)
    rec = np.zeros((len(n), 8), F32)
    rec[:, 0:3] = F32(0.7)
    rec[n[:, 0] > F32(0.99), 0:3] = (1, 0, 0)
    rec[~(n[:, 0] > F32(0.99)) & (-n[:, 0] > F32(0.99)), 0:3] = (0, 1, 0)
    return rec


# ------------------------------------------------------------------------------------------ the walker
def walk_nee_sphere(O, scene, W, H, segments, rec, lights, sphere, frame=0, rows=None, spp=1):
    """nee_paths.walk_nee with the sphere sample where `sphere`: dict of IMAGE [H, W, 4], HIT_ID [H, W], rays (the sphere sample
    sends none), nee_paths' counts of the triangle samples, and of the sphere's: sphere_samples, sphere_taken, sphere_valid,
    sphere_dropped / sphere_kept (paths that met the light behind the first segment with the sphere bit set / clear)"""
    cfg = P.configure(O.config_default(W, H), scene, segments, spp)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(scene), frame)
    y0, y1 = rows or (0, H)
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(W), indexing="ij")
    xs, ys = xs.ravel().astype(U32), ys.ravel().astype(U32)
    k = len(xs)
    seeds = np.stack([xs, ys, np.full(k, pc.frameNumber, U32), np.full(k, pc.sample_batch, U32)], 1)
    rng = O.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds, U32))[:, 0].copy()          # :297
    total, first_id = np.zeros((k, 3), F32), None
    count = dict(rays=0, samples=0, queries=0, lit=0, kept=0, dropped=0, sphere_samples=0, sphere_taken=0, sphere_valid=0,
                 sphere_dropped=0, sphere_kept=0)
    lights = np.ascontiguousarray(lights, U32)
    for _ in range(spp):
        rng, d = _primary(O, cfg, rng, xs, ys)
        value, rng, ids = _path(O, cfg, pc, scene, np.ascontiguousarray(rec, F32), lights, bool(sphere), rng, d, count)
        total = (total + value).astype(F32)                                                                  # :325
        first_id = ids if first_id is None else first_id
    image = np.zeros((H, W, 4), F32)
    hit_id = np.zeros((H, W), U32)
    image[y0:y1, :, :3] = (total / F32(spp)).astype(F32).reshape(y1 - y0, W, 3)                              # :328
    hit_id[y0:y1] = first_id.reshape(y1 - y0, W)
    return dict(IMAGE=image, HIT_ID=hit_id, **count)


def _path(O, cfg, pc, scene, rec, lights, sphere, rng, d, count):
    """one sample's paths from the camera along d [k, 3]: (R + terminal colour [k, 3], rng state [k], first hit id [k])"""
    tris = np.ascontiguousarray(scene.tris, F32)
    n_base, segments, k, L = len(rec), int(cfg.max_segments), len(d), len(lights)
    rng = rng.copy()
    light_c = F32(list(pc.lightPos))
    light_col = (F32(list(pc.currentCameraColor)) * F32(cfg.light_intensity)).astype(F32)                   # :281
    light_first = (light_col / F32(cfg.first_hit_light_divisor)).astype(F32)                                 # :229
    radius, ray_offset, tmax = F32(cfg.light_radius), F32(cfg.ray_offset), float(cfg.ray_tmax)
    r2 = r2_of(radius)
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
        acc[j] = (acc[j] * m[:, 0:3]).astype(F32)                                                    # :244
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
            id1 = lights[N.pick(u_l, np.full(len(q), L))]
            lt = tris[id1.astype(np.int64) - 1]
            s = N.sample32(O, N.cases_of(lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, nf[q], u_l, u_a, u_b, L))[:, :8].view(F32)
            ke = rec[(id1.astype(np.int64) - 1) % n_base, 4:7]
            gain = (((acc[jq] * ke).astype(F32)) * s[:, 6:7]).astype(F32)                             # (T * Ke) * g
            valid = s[:, 7] != 0
            seen, _, _ = _closest_hits(O, tris, x[valid], s[valid, 3:6], tmax)
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
            s = sphere32(O, cases_of(x, nf[q], light_c, r2, u_c, u_p)).view(F32)
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
            nm, dm, g = nf[mirror], dd[mirror], np.abs(w[mirror])
            c2 = (F32(-2.0) * dot(O, nm, dm)).astype(F32)
            refl = fma(O, c2[:, None], nm, dm)
            sph = np.stack([(rho[mirror] * cs[mirror]).astype(F32), (rho[mirror] * sn[mirror]).astype(F32), u[mirror]], 1)
            lobe = normalize(O, fma(O, g[:, None], sph, refl))
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


# ------------------------------------------------------------------------------------------ scenes
NEAR_LIGHT = (0.3, -0.2, 0.9)                    # a moderate distance above the receiver's plane z = 0
LOW_LIGHT = (0.3, -0.2, 0.1)                     # centre 0.1 above the plane, radius 0.2: the sphere comes through the floor
ROOM_LIGHT = (1.0, 0.2, -1.5)                    # inside the glass room, beside its box
MOVED_LIGHT = (-0.4, 0.3, 0.7)                   # where the second frame of the sequence has the near light


def receiver_near():
    """nee_scenes.receiver() with the sphere light at a moderate distance above the receiver"""
    return N.receiver()._replace(name="receiver_near", light=NEAR_LIGHT)


def receiver_low():
    """... with the light's centre 0.1 above the plane: hit points lie inside the sphere and on it, cones are cut by the horizon"""
    return N.receiver()._replace(name="receiver_low", light=LOW_LIGHT)


def receiver_moved():
    return N.receiver()._replace(name="receiver_moved", light=MOVED_LIGHT)


def glass_room_lit(form="small"):
    """dielectric_scenes.glass_room with the light inside the room: (scene, glass)"""
    scene, glass = DS.glass_room(form)
    return scene._replace(name="glass_room_lit", light=ROOM_LIGHT), glass


def three_ends_plain():
    """pathtrace_scenes.three_ends, which has a near light, without its material table: the normal-keyed colours"""
    return P.three_ends("small")._replace(name="three_ends_plain", tri_material=None, materials=None)
