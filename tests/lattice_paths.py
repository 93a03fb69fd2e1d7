"""One numpy float32 path walker for the whole shading lattice of K2 (csrc/shade_segment.hpp, csrc/pathtrace_tile.hpp): TEX 0 / 1 / 2
x DEMOD x SPEC 0 .. 6, for test_lattice_*.py.

walk() is nee_power.walk_nee_power's loop — diffuse, glossy, mirror and dielectric bounces, emitters, the uniform and the weighted
pick of the light list, the sphere sample, samples per pixel — composed with what that walker leaves out:

  real mip levels   a hit on a texture with RTPT_TEX_MIPMAP is sampled at the level of its ray's footprint:
                    texture_mip_scenes.footprint_lod32(w, dot(n, d), the posed vertices, the uv record, W, H) with w = t x
                    primary_spread(slope, frame height) at segment 0 and t x BOUNCE_SPREAD behind it, clamp_lod, sample_lod over the
                    texture's chain.  t is the closest hit's (oracle_closest_hit's, which oracle_raytrace_ext takes too), n the STORED
                    normal before faceforward, d the incoming direction — the refracted one inside or behind glass.  A texture
                    without the flag, and every texture of an atlas without any flag (TEX = 1), reads level 0 (texture_scenes.sample)
  the ALBEDO plane  demod: at segment 0 the hit's albedo (record colour x texel) goes to ALBEDO and not into the throughput; a path
                    that ends at segment 0 on the light, the sky or an emitter stores (1, 1, 1) and keeps its colour; the fourth
                    channel is 0.  The light samples' gains take the throughput as it then is, without the albedo
  hit records       hits=[]: one dict of arrays per shaded segment (pixel, segment, ray, id, level, albedo, ...), for the float64
                    replay of tests/test_lattice_cpu.py
  records per posed triangle   a scene without a material table walks with nee_sphere.normal_keyed_records, one record per POSED
                    triangle (the colour follows the posed normal), while its textures stay per BASE triangle: the material record
                    is (id - 1) % len(rec), the texture record (id - 1) % len(tri_texture)

tests/test_lattice_cpu.py holds it to the C oracle (SPEC 0 / 1, every TEX, DEMOD), to walk_nee_power and dielectric_scenes.walk
(level 0), and to float64, before tests/test_lattice_gpu.py judges a GPU frame by it."""
import ctypes as C
from collections import namedtuple

import numpy as np

import contract_cases as CC
import nee_power as PW
import nee_scenes as N
import nee_sphere as NS
import pathtrace_scenes as P
import shading_scenes as SS
import texture_mip_scenes as MS
import texture_scenes as TS
from dielectric_scenes import _contract, _primary, _rng_next, dot, fma, interface32, normalize
from gbuffer_scenes import fill_push_constants

F32, U32 = np.float32, np.uint32

# what rtpt_scene_set_textures takes (per BASE triangle: tri_uv [b, 6], tri_texture [b]; desc [n, 4], texels [m, 4]) and, per
# texture, the levels the device samples (chains[k]: a list of [h, w, 4]; one level where the texture has no mip flag).
# chains None: the atlas has no mip flag at all and the launch is TEX = 1
Tex = namedtuple("Tex", "tri_uv tri_texture desc texels chains")


def textures(sh, mode, given=None):
    """the Tex of a shading_scenes.Shading.  mode 0: None; 1: its atlas without any mip flag; 2: the mixed atlas, whose flagged
    textures get the chain the device generates (MS.build_chain); given: chains handed over whole (SS.given_atlas)"""
    if not mode:
        return None
    if given is not None:
        desc, texels = SS.given_atlas(sh, given)
        return Tex(sh.tri_uv, sh.tri_texture, desc, texels, [list(c) for c in given])
    desc, texels = SS.atlas(sh, mode)
    chains = None
    if (desc[:, 3] & MS.MIPMAP).any():
        chains = [MS.build_chain(im) if f & MS.MIPMAP else [np.asarray(im, F32)] for im, f in zip(sh.images, desc[:, 3].tolist())]
    return Tex(sh.tri_uv, sh.tri_texture, desc, texels, chains)


def closest_hits(O, tris, o, d, tmax):
    """oracle_closest_hit per ray: (id [k] uint32, t [k], b1 [k], b2 [k]); t, b1, b2 are 0 where nothing is hit"""
    lib = O.lib()
    tris = np.ascontiguousarray(tris, F32)
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    k = len(o)
    ids, ts, b1s, b2s = np.zeros(k, U32), np.zeros(k, F32), np.zeros(k, F32), np.zeros(k, F32)
    t, b1, b2 = C.c_float(), C.c_float(), C.c_float()
    tp, n, tm = C.c_void_p(tris.ctypes.data), C.c_uint32(len(tris)), C.c_float(tmax)
    ob, db = o.ctypes.data, d.ctypes.data
    fn = lib.oracle_closest_hit
    for i in range(k):
        ids[i] = fn(tp, n, C.c_void_p(ob + 12 * i), C.c_void_p(db + 12 * i), tm, C.byref(t), C.byref(b1), C.byref(b2))
        if ids[i]:
            ts[i], b1s[i], b2s[i] = t.value, b1.value, b2.value
    return ids, ts, b1s, b2s


def _texels(O, tex, base, b0, b1, b2, t, nd, p, spread):
    """(rgb [k, 3] the hits multiply their colour by — 1 where untextured —, level [k] as clamped to the chain, textured [k],
    mipped [k]: the texture has the flag and more than one level) of hits on base triangles `base` with barycentrics b, hit
    distance t, nd = dot(stored normal, incoming direction) and posed vertices p [k, 3, 3]"""
    uv6 = np.asarray(tex.tri_uv, F32).reshape(-1, 6)[base]
    ti = np.asarray(tex.tri_texture, np.int64)[base]
    k = len(base)
    out, lam_out, mipped = np.ones((k, 3), F32), np.zeros(k, F32), np.zeros(k, bool)
    u = fma(O, b2, uv6[:, 4], fma(O, b1, uv6[:, 2], (b0 * uv6[:, 0]).astype(F32)))
    v = fma(O, b2, uv6[:, 5], fma(O, b1, uv6[:, 3], (b0 * uv6[:, 1]).astype(F32)))
    desc = np.asarray(tex.desc).reshape(-1, 4)
    for tx in np.unique(ti[ti > 0]):
        sel = ti == tx
        uv = np.stack([u[sel], v[sel]], 1)
        w_, h_, _, flags = (int(x) for x in desc[tx - 1])
        if tex.chains is None:                                        # TEX = 1: tex::sample
            out[sel] = TS.sample(tex.texels, desc[tx - 1], uv)[:, :3]
            continue
        chain = tex.chains[tx - 1]
        lam = np.zeros(int(sel.sum()), F32)
        if flags & MS.MIPMAP:                                         # hit_texture_lod
            w = (t[sel] * F32(spread)).astype(F32)
            lam = MS.footprint_lod32(w, nd[sel], p[sel], uv6[sel], w_, h_)
            mipped[sel] = len(chain) > 1
        out[sel] = MS.sample_lod(chain, flags, uv, lam)[:, :3]        # tex::sample_lod (lambda 0 without the flag: level 0)
        lam_out[sel] = MS.clamp_lod(lam, len(chain))
    return out, lam_out, ti > 0, mipped


COUNTS = ("rays", "samples", "queries", "lit", "kept", "dropped", "sphere_samples", "sphere_taken", "sphere_valid", "sphere_dropped",
          "sphere_kept", "transmitted", "reflected", "mip_behind", "lod_fraction", "lod_fraction_behind")


def walk(O, scene, W, H, segments, rec, lights=(), sphere=False, power=False, frame=0, rows=None, spp=1, tex=None, demod=False,
         hits=None):
    """K2 of `scene` (scene.tris: the posed triangles; rec: one record per base triangle, or per posed triangle for a scene
    without a table) over the light list `lights`: dict of IMAGE [H, W, 4], HIT_ID [H, W], ALBEDO [H, W, 4] where demod, rays,
    seq_n [H, W] (the closest-hit queries of the pixel's last sample's path, shadow rays not counted), nee_power's counts and picks, and
      transmitted / reflected     dielectric hits that bounced, by the side they left on
      mip_behind                  hits on a mip-mapped texture of paths that met a dielectric at an earlier segment
      lod_levels, lod_fraction    distinct integer parts of the level, and hits with a fractional level, among such hits at segment >= 1
      lod_levels_behind, lod_fraction_behind   the same among those behind a dielectric
    rows [y0, y1) computed; the planes are full frames"""
    assert not (demod and spp > 1), "rtpt_create refuses the two together"
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
    count = {c: 0 for c in COUNTS}
    count.update(picks=np.zeros(len(lights), np.int64), levels=set(), levels_behind=set())
    rec = np.ascontiguousarray(rec, F32)
    cdf = PW.table(PW.weights(O, scene.tris, rec, lights)) if power and len(lights) else None
    albedo = np.zeros((k, 4), F32)
    albedo[:, :3] = 1
    seq_n = np.zeros(k, np.int32)
    for smp in range(spp):
        rng, d = _primary(O, cfg, rng, xs, ys)
        value, rng, ids = _path(O, cfg, pc, scene, rec, lights, cdf, bool(sphere), rng, d, count, tex, H, albedo if demod else None,
                                seq_n, hits, smp, xs, ys)
        total = (total + value).astype(F32)                                                                  # :325
        first_id = ids if first_id is None else first_id
    image = np.zeros((H, W, 4), F32)
    hit_id = np.zeros((H, W), U32)
    image[y0:y1, :, :3] = (total / F32(spp)).astype(F32).reshape(y1 - y0, W, 3)                              # :328
    hit_id[y0:y1] = first_id.reshape(y1 - y0, W)
    out = dict(IMAGE=image, HIT_ID=hit_id)
    if demod:
        out["ALBEDO"] = np.zeros((H, W, 4), F32)
        out["ALBEDO"][y0:y1] = albedo.reshape(y1 - y0, W, 4)
    out["seq_n"] = np.zeros((H, W), np.int32)
    out["seq_n"][y0:y1] = seq_n.reshape(y1 - y0, W)
    count["lod_levels"], count["lod_levels_behind"] = len(count.pop("levels")), len(count.pop("levels_behind"))
    out.update(count)
    return out


def _path(O, cfg, pc, scene, rec, lights, cdf, sphere, rng, d, count, tex, frame_h, albedo, seq_n, hits, smp, xs, ys):
    """nee_power._path, statement for statement, but for the texel's level, the ALBEDO plane (albedo [k, 4], None: not
    demodulated), the records and the counts"""
    tris = np.ascontiguousarray(scene.tris, F32)
    n_base, segments, k, L = len(rec), int(cfg.max_segments), len(d), len(lights)
    rng = rng.copy()
    light_c = F32(list(pc.lightPos))
    light_col = (F32(list(pc.currentCameraColor)) * F32(cfg.light_intensity)).astype(F32)                   # :281
    light_first = (light_col / F32(cfg.first_hit_light_divisor)).astype(F32)                                 # :229
    radius, ray_offset, tmax = F32(cfg.light_radius), F32(cfg.ray_offset), float(cfg.ray_tmax)
    r2 = NS.r2_of(radius)
    spread0 = MS.primary_spread(cfg.fov_slope, frame_h)      # (2.0f * slope) / (float)H of the FULL frame
    o = np.broadcast_to(F32(scene.cam), (k, 3)).astype(F32).copy()
    d = d.copy()
    acc = np.ones((k, 3), F32)
    radiance = np.zeros((k, 3), F32)                  # R: restarts at 0 with every sample
    sampled = np.zeros(k, bool)                       # the sampled bit (emissive triangles)
    sbit = np.zeros(k, bool)                          # the sphere bit: the primary ray starts with both clear
    glassed = np.zeros(k, bool)                       # the path met a dielectric at an earlier segment
    alive = np.ones(k, bool)
    first_id = np.zeros(k, U32)
    seq_n[:] = 0
    for seg in range(segments):
        idx = np.flatnonzero(alive)
        if not len(idx):
            break
        oo, dd = o[idx], d[idx]
        ids, th, b1, b2 = closest_hits(O, tris, oo, dd, tmax)
        count["rays"] += len(idx)
        seq_n[idx] += 1
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
        hid = ids[hit][keep].astype(np.int64) - 1
        th, b1, b2, dd, oo = th[hit][keep], b1[hit][keep], b2[hit][keep], dd[hit][keep], oo[hit][keep]
        b0 = ((F32(1.0) - b1).astype(F32) - b2).astype(F32)                                          # :134
        tri = tris[hid]
        e1, e2 = (tri[:, 3:6] - tri[:, 0:3]).astype(F32), (tri[:, 6:9] - tri[:, 0:3]).astype(F32)
        n = normalize(O, _contract(O, "cross", e1, e2))                                              # :150, the stored normal
        alb = m[:, 0:3]
        lam, textured, mipped = np.zeros(len(j), F32), np.zeros(len(j), bool), np.zeros(len(j), bool)
        if tex is not None:
            texel, lam, textured, mipped = _texels(O, tex, hid % len(tex.tri_texture), b0, b1, b2, th, dot(O, n, dd), tri.reshape(-1, 3, 3),
                                                   spread0 if seg == 0 else MS.BOUNCE_SPREAD)
            alb = (alb * texel).astype(F32)
        if albedo is not None and seg == 0:           # demodulated: into the plane, not into the throughput
            albedo[j, :3] = alb
        else:
            acc[j] = (acc[j] * alb).astype(F32)                                                      # :244
        count["mip_behind"] += int((mipped & glassed[j]).sum())
        if seg > 0:
            for key, sel in (("", mipped), ("_behind", mipped & glassed[j])):
                count["levels" + key] |= set(np.floor(lam[sel]).astype(int).tolist())
                count["lod_fraction" + key] += int((lam[sel] % 1 != 0).sum())
        if hits is not None:
            hits.append(dict(x=xs[j].copy(), y=ys[j].copy(), sample=np.full(len(j), smp), seg=np.full(len(j), seg), o=oo, d=dd, id=hid + 1,
                             lod=lam, albedo=alb, textured=textured, mipped=mipped, behind=glassed[j].copy()))
        if seg + 1 >= segments:                       # the last segment: no light draw, no shadow query; the bounce's two draws
            rng[j] = _rng_next(O, _rng_next(O, rng[j])[0])[0]      # only move the stream (:256-257)
            break
        pos = fma(O, tri[:, 6:9], b2[:, None], fma(O, tri[:, 3:6], b1[:, None], (tri[:, 0:3] * b0[:, None]).astype(F32)))   # :137
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
            count["picks"] += np.bincount(entry, minlength=L)
            ke = rec[(id1.astype(np.int64) - 1) % n_base, 4:7]
            gain = (((acc[jq] * ke).astype(F32)) * g[:, None]).astype(F32)                            # (T * Ke) * g
            seen, _, _, _ = closest_hits(O, tris, x[valid], wd[valid], tmax)
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
            count["transmitted"] += int(transmitted.sum())
            count["reflected"] += int((~transmitted).sum())
            glassed[j[glass]] = True
        o[j] = fma(O, off[:, None], nf, pos)                                                          # :250
        d[j] = dn
    return (radiance + acc).astype(F32), rng, first_id                                                # R + terminal


def hit_table(hits):
    """the walker's hit records, one array per key over every shaded hit of the frame"""
    return {k: np.concatenate([h[k] for h in hits]) for k in hits[0]} if hits else {}
