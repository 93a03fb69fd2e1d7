"""The light list and a numpy float32 path walker with next-event estimation (RTPT_FLAG_EXT_NEE; csrc/light_sample.hpp states the
rules) for test_nee_paths_*.py.

light_list restates csrc/light_list_host.hpp.  walk_nee restates dielectric_scenes._path's loop — K2 for materials without
textures — with the light sample at every diffuse hit that is not a path's last segment, from the pieces dielectric_scenes exports
(_primary, _closest_hits, _rng_next, records, interface32) and nee_scenes.sample32.  With an empty list it takes no light draw and
is dielectric_scenes.walk, which tests/test_nee_paths_cpu.py asks for bit by bit before anything else is concluded from it.
With `texture` it multiplies every hit's albedo by the texel texture_scenes.sample reads at the hit's interpolated uv (level 0:
textures without a mip chain, or constant images, whose every level holds the same value)."""
from functools import lru_cache

import numpy as np

import contract_cases as CC
import dielectric_scenes as DS
import nee_scenes as N
import pathtrace_scenes as P
import texture_scenes as TS
from dielectric_scenes import _closest_hits, _contract, _primary, _rng_next, dot, fma, interface32, normalize, records  # noqa: F401
from gbuffer_scenes import fill_push_constants

F32, U32 = np.float32, np.uint32


# ------------------------------------------------------------------------------------------ the light list
def light_list(scene, n_instances=1, rec=None):
    """uint32 [L]: id + 1 of every posed triangle inst * n_base + t whose base triangle's record is emissive, ascending.  rec: the
    per-base-triangle records (dielectric_scenes.records) where some material is specular or dielectric; else the scene's own"""
    rec = records(scene) if rec is None else np.asarray(rec, F32)
    t = np.flatnonzero(rec[:, 7] != 0).astype(np.int64)
    n_base = len(rec)
    ids = (np.arange(n_instances, dtype=np.int64)[:, None] * n_base + t[None, :] + 1).ravel()
    return ids.astype(U32)


# ------------------------------------------------------------------------------------------ the walker
def walk_nee(O, scene, W, H, segments, rec, lights, frame=0, rows=None, spp=1, texture=None):
    """K2 of `scene` (scene.tris: the posed triangles, every instance's; rec: one record per BASE triangle) with next-event
    estimation over the list `lights` (id + 1 of posed triangles; empty: none is sampled, the walk is dielectric_scenes.walk's):
    dict of IMAGE [H, W, 4], HIT_ID [H, W], rays, and of the light samples taken: samples, queries (valid ones: a shadow ray each)
    and lit (those that reached their light), kept and dropped (emitters met behind the first segment with the sampled bit clear
    / set); rows [y0, y1) computed.  texture: (tri_uv [t, 6], tri_texture [t], textures [n, 4], texels [m, 4]) per BASE triangle, as
    rtpt_scene_set_textures takes them"""
    cfg = P.configure(O.config_default(W, H), scene, segments, spp)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(scene), frame)
    y0, y1 = rows or (0, H)
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(W), indexing="ij")
    xs, ys = xs.ravel().astype(U32), ys.ravel().astype(U32)
    k = len(xs)
    seeds = np.stack([xs, ys, np.full(k, pc.frameNumber, U32), np.full(k, pc.sample_batch, U32)], 1)
    rng = O.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds, U32))[:, 0].copy()          # :297
    total, first_id = np.zeros((k, 3), F32), None
    count = dict(rays=0, samples=0, queries=0, lit=0, kept=0, dropped=0)
    lights = np.ascontiguousarray(lights, U32)
    for _ in range(spp):
        rng, d = _primary(O, cfg, rng, xs, ys)
        value, rng, ids = _path_nee(O, cfg, pc, scene, np.ascontiguousarray(rec, F32), lights, rng, d, count, texture)
        total = (total + value).astype(F32)                                                                  # :325
        first_id = ids if first_id is None else first_id
    image = np.zeros((H, W, 4), F32)
    hit_id = np.zeros((H, W), U32)
    image[y0:y1, :, :3] = (total / F32(spp)).astype(F32).reshape(y1 - y0, W, 3)                              # :328
    hit_id[y0:y1] = first_id.reshape(y1 - y0, W)
    return dict(IMAGE=image, HIT_ID=hit_id, **count)


def _texels(O, texture, base, b0, b1, b2):
    """rgb [k, 3] the hits on base triangles `base` with barycentrics b multiply their albedo by (1 where untextured)"""
    tri_uv, tri_texture, desc, texels = texture
    uv6 = np.asarray(tri_uv, F32).reshape(-1, 6)[base]
    ti = np.asarray(tri_texture, np.int64)[base]
    out = np.ones((len(base), 3), F32)
    u = fma(O, b2, uv6[:, 4], fma(O, b1, uv6[:, 2], (b0 * uv6[:, 0]).astype(F32)))
    v = fma(O, b2, uv6[:, 5], fma(O, b1, uv6[:, 3], (b0 * uv6[:, 1]).astype(F32)))
    for t in np.unique(ti[ti > 0]):
        sel = ti == t
        out[sel] = TS.sample(texels, np.asarray(desc).reshape(-1, 4)[t - 1], np.stack([u[sel], v[sel]], 1))[:, :3]
    return out


def _path_nee(O, cfg, pc, scene, rec, lights, rng, d, count, texture=None):
    """one sample's paths from the camera along d [k, 3]: (R + terminal colour [k, 3], rng state [k], first hit id [k]); the
    closest-hit queries, shadow rays included, are added to count["rays"]"""
    tris = np.ascontiguousarray(scene.tris, F32)
    n_base, segments, k, L = len(rec), int(cfg.max_segments), len(d), len(lights)
    rng = rng.copy()
    light_c = F32(list(pc.lightPos))
    light_col = (F32(list(pc.currentCameraColor)) * F32(cfg.light_intensity)).astype(F32)                   # :281
    light_first = (light_col / F32(cfg.first_hit_light_divisor)).astype(F32)                                 # :229
    radius, ray_offset, tmax = F32(cfg.light_radius), F32(cfg.ray_offset), float(cfg.ray_tmax)
    o = np.broadcast_to(F32(scene.cam), (k, 3)).astype(F32).copy()
    d = d.copy()
    acc = np.ones((k, 3), F32)
    radiance = np.zeros((k, 3), F32)                  # R: restarts at 0 with every sample
    sampled = np.zeros(k, bool)                       # the sampled bit: the primary ray starts with it clear
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
        acc[idx[lit]] = (acc[idx[lit]] * (light_first if seg == 0 else light_col)).astype(F32)       # :229, :233: never sampled
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
            alb = (alb * _texels(O, texture, (ids[hit][keep].astype(np.int64) - 1) % n_base, b0, b1, b2)).astype(F32)
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
        if L:                                         # ---- the light sample (light_sample.hpp), at the diffuse hits
            q = np.flatnonzero(diffuse)
            jq = j[q]
            x = fma(O, ray_offset, nf[q], pos[q])                                                     # :250, the bounce's origin
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
            jl = jq[valid][reached]
            radiance[jl] = (radiance[jl] + gain[valid][reached]).astype(F32)
            count["rays"] += int(valid.sum())
            count["samples"] += len(q)
            count["queries"] += int(valid.sum())
            count["lit"] += int(reached.sum())
            sampled[jq] = True                        # valid or not
            sampled[j[~diffuse]] = False              # a specular or dielectric hit clears the bit
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
OCCLUDER = np.array([(0.2, -1.0, 0.8), (1.4, -1.0, 0.8), (1.4, 0.6, 0.8), (0.2, 0.6, 0.8)], np.float64)
SMALL_LAMP = np.array([(-1.8, 0.4, 1.5), (-1.5, 0.4, 1.5), (-1.5, 0.8, 1.5), (-1.8, 0.8, 1.5)], np.float64)
SMALL_LAMP_KE = (1.0, 6.0, 3.0)


def _receiver_quads():
    return [[(-2.3, -1.8, 0.0), (2.3, -1.8, 0.0), (2.3, 1.8, 0.0), (-2.3, 1.8, 0.0)], N.RECEIVER_LAMP]


@lru_cache(maxsize=None)
def occluder():
    """nee_scenes.receiver() plus one opaque diffuse quad in the plane z = 0.8, between part of the receiver and the lamp (z = 2) and
    inside the view: pixels whose light samples it stops get no direct term.  Materials: 0 the receiver, 1 the occluder, 2 the lamp"""
    quads = np.array(_receiver_quads()[:1] + [OCCLUDER] + [N.RECEIVER_LAMP], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1, 2]))
    materials = P._materials((N.RECEIVER_KD, (0.25, 0.5, 0.125)), (N.RECEIVER_KE,))
    return P.Scene("nee_occluder", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)


@lru_cache(maxsize=None)
def two_lamps():
    """the receiver under two lamps of unequal area and colour — the trapezoid and a small quad on the other side, nearer — and one
    DEGENERATE emissive triangle (three points on a line): it is in the list, its samples are never valid and no ray hits it.
    Materials: 0 the receiver, 1 the trapezoid, 2 the small lamp and the degenerate triangle"""
    quads = np.array(_receiver_quads() + [SMALL_LAMP], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1, 2]))
    line = np.array([[0.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0]], F32)
    tris = P._frozen(np.concatenate([np.asarray(tris, F32).reshape(-1, 9), line]))
    mat = P._frozen(np.concatenate([np.asarray(mat), [2]]).astype(np.asarray(mat).dtype))
    materials = P._materials((N.RECEIVER_KD,), (N.RECEIVER_KE, SMALL_LAMP_KE))
    return P.Scene("nee_two_lamps", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)


def translated(scene, offsets):
    """the scene's mesh as len(offsets) instances, instance i moved by offsets[i]: (instance transforms [n, 12] float32, the posed
    scene the walker takes — every instance's triangles, one record per base triangle).  A translation poses a vertex as v + t, one
    rounding, which is what the flatten's fused arithmetic gives for rows of the identity"""
    base = np.asarray(scene.tris, F32).reshape(-1, 3, 3)
    xf = np.zeros((len(offsets), 3, 4), F32)
    xf[:, 0, 0] = xf[:, 1, 1] = xf[:, 2, 2] = 1
    xf[:, :, 3] = F32(offsets)
    posed = np.concatenate([(base + F32(t)[None, None, :]).astype(F32) for t in offsets]).reshape(-1, 9)
    return xf.reshape(-1, 12), scene._replace(name=scene.name + "_x%d" % len(offsets), tris=P._frozen(posed))
