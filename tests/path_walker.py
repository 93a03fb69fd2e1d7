"""The one numpy float32 path walker of the tests: K2's path segment (csrc/shade_segment.hpp, csrc/pathtrace_tile.hpp) restated once,
for every test_*_cpu.py / test_*_gpu.py that judges a traced frame.

walk() is primary-ray generation and the segment loop over the contract functions (oracle.contract_array), with oracle_closest_hit
through ctypes for id, t, b1 and b2 of every ray.  Every shading feature is a keyword of walk() and a marked block of _path():

  (always)   diffuse, glossy, mirror and dielectric bounces, emitters, the sphere light and the sky, samples per pixel
  TEX        tex: a Tex — level 0 where its chains are None (tex::sample), else the level of the ray's footprint:
             texture_mip_scenes.footprint_lod32(w, dot(n, d), the posed vertices, the uv record, W, H) with w = t x
             primary_spread(slope, frame height) at segment 0 and t x BOUNCE_SPREAD behind it, clamp_lod, sample_lod over the
             texture's chain.  t is the closest hit's, n the STORED normal before faceforward, d the incoming direction
  DEMOD      demod: at segment 0 the hit's albedo (record colour x texel) goes to ALBEDO and not into the throughput; a path that
             ends at segment 0 on the light, the sky or an emitter stores (1, 1, 1) and keeps its colour; the fourth channel is 0
  NEE        lights: the list of emissive posed triangles (id + 1), sampled at every diffuse hit that is not a path's last segment;
             power: picked by weight (nee_power) and not uniformly (nee_scenes)
  SPHERE     sphere: the analytic sphere light sampled at the same hits (nee_sphere)
  MIS        mis: the power heuristic between the triangle sample and the bounce that runs into an emitter (nee_mis)
  NRM        normals: a normal_paths.Normals — interpolated vertex normals and the side tests of csrc/shading_normal.hpp

The rule functions stay in the feature modules, where the selftest kernels are held to them operand by operand; this module only
imports them, and no feature module imports this one.  A material record is (id - 1) % len(rec) — one per base triangle, or per
POSED triangle for a scene without a table (nee_sphere.normal_keyed_records) —, a texture record (id - 1) % len(tri_texture).

What holds the walker: tests/test_dielectric_cpu.py and tests/test_lattice_cpu.py pin it to the C oracle bit for bit where the oracle
knows the feature, the float64 replays of test_lattice_cpu.py and test_normal_paths_cpu.py to exact arithmetic, and six tests to
tests/golden/walker_frames.npz — the frames of the seven walkers this one replaced (recorded(); DESIGN.md, "The test walker")."""
import ctypes as C
import hashlib
import os
from collections import namedtuple
from functools import lru_cache

import numpy as np

import contract_cases as CC
import nee_mis as NM
import nee_power as PW
import nee_scenes as N
import nee_sphere as NS
import pathtrace_scenes as P
import shading_scenes as SS
import texture_mip_scenes as MS
import texture_scenes as TS
from dielectric_scenes import _contract, _primary, _rng_next, dot, fma, normalize
from gbuffer_scenes import fill_push_constants
from normal_paths import absorbed, dielectric_offset, hit_shading_normal, interface_faced, sample_side

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


# the integer counts of walk()'s result, each 0 where its feature is off (but kept and sphere_kept: see walk())
COUNTS = ("rays", "samples", "queries", "lit", "kept", "dropped", "sphere_samples", "sphere_taken", "sphere_valid", "sphere_dropped",
          "sphere_kept", "transmitted", "reflected", "mip_behind", "lod_fraction", "lod_fraction_behind", "smooth", "fallback4",
          "fallback7", "flipped", "absorbed", "side_invalid", "offset_changed", "weighted")


def walk(O, scene, W, H, segments, rec, lights=(), sphere=False, power=False, mis=False, normals=None, n_base=None,
         tex=None, demod=False, frame=0, frames=None, rows=None, spp=1, hits=None):
    """K2 of `scene` (scene.tris: the posed triangles, every instance's; rec: dielectric_scenes.records per base triangle, or
    per posed triangle for a scene without a table) over the light list `lights`; n_base: the base triangle count of `normals` where
    rec is per POSED triangle.  A dict of IMAGE [H, W, 4], HIT_ID [H, W], ALBEDO [H, W, 4] where demod, seq_n [H, W] (the
    closest-hit queries of the pixel's last sample's path, shadow rays not counted), picks [L] (draws per entry of the list) and
      rays                          closest-hit queries, shadow rays included
      samples, queries, lit         triangle samples taken, the valid ones (a shadow ray each), those that reached their light
      kept, dropped                 emitters met behind the first segment with the sampled bit clear / set (kept and sphere_kept
                                    count without a sample too: the bit is then always clear)
      weighted, wb_min, wb_max      with `mis`: the dropped ones, which end the path with (T * Ke) * wb and not with 0, and the
                                    smallest and largest wb among them (1, 0 where there was none)
      sphere_samples, sphere_taken, sphere_valid, sphere_dropped, sphere_kept   the same of the sphere sample and the sphere bit
      transmitted, reflected        dielectric hits that bounced, by the side they left on
      mip_behind                    hits on a mip-mapped texture of paths that met a dielectric at an earlier segment
      lod_levels, lod_fraction      distinct integer parts of the level, and hits with a fractional level, among such hits at segment >= 1
      lod_levels_behind, lod_fraction_behind   the same among those behind a dielectric
      smooth, fallback4, fallback7, flipped    hits shaded with ns; rule 4 / rule 7 fell back; rule 6
      absorbed, side_invalid, offset_changed   side test 1; side test 2 refused a sample the sample's own test allowed; side test 3
                                    chose another sign than `transmitted`
    rows [y0, y1) computed; the planes are full frames.  frames: a sequence of frame numbers walked as one batch of paths (a path's
    stream depends on its pixel and its frame number only); every plane then has len(frames) in front, and `frame` is not read.
    hits=[]: one dict of arrays per shaded segment is appended (hit_table), for the float64 replays"""
    assert not (demod and spp > 1), "rtpt_create refuses the two together"
    cfg = P.configure(O.config_default(W, H), scene, segments, spp)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(scene), frame)
    y0, y1 = rows or (0, H)
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(W), indexing="ij")
    xs, ys = xs.ravel().astype(U32), ys.ravel().astype(U32)
    fr = np.asarray([pc.frameNumber] if frames is None else list(frames), U32)
    xs, ys, fn = np.tile(xs, len(fr)), np.tile(ys, len(fr)), np.repeat(fr, len(xs))
    k = len(xs)
    seeds = np.stack([xs, ys, fn, np.full(k, pc.sample_batch, U32)], 1)
    rng = O.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds, U32))[:, 0].copy()          # :297
    total, first_id = np.zeros((k, 3), F32), None
    lights = np.ascontiguousarray(lights, U32)
    count = {c: 0 for c in COUNTS}
    count.update(picks=np.zeros(len(lights), np.int64), levels=set(), levels_behind=set(), wb_min=1.0, wb_max=0.0)
    rec = np.ascontiguousarray(rec, F32)
    cdf = PW.table(PW.weights(O, scene.tris, rec, lights)) if power and len(lights) else None
    albedo = np.zeros((k, 4), F32)
    albedo[:, :3] = 1
    seq_n = np.zeros(k, np.int32)
    nb = int(n_base if n_base is not None else (len(normals.tri_smooth) if normals is not None else len(rec)))
    for smp in range(spp):
        rng, d = _primary(O, cfg, rng, xs, ys)
        value, rng, ids = _path(O, cfg, pc, scene, rec, lights, cdf, bool(sphere), bool(mis) and len(lights) > 0, normals, nb, tex, H,
                                rng, d, count, albedo if demod else None, seq_n, hits, smp, xs, ys)
        total = (total + value).astype(F32)                                                                  # :325
        first_id = ids if first_id is None else first_id

    def plane(values, dtype, *channels):
        full = np.zeros((len(fr), H, W) + channels, dtype)
        full[:, y0:y1] = values.reshape((len(fr), y1 - y0, W) + channels)
        return full[0] if frames is None else full

    out = dict(IMAGE=plane(np.concatenate([(total / F32(spp)).astype(F32), np.zeros((k, 1), F32)], 1), F32, 4),    # :328
               HIT_ID=plane(first_id, U32))
    if demod:
        out["ALBEDO"] = plane(albedo, F32, 4)
    out["seq_n"] = plane(seq_n, np.int32)
    count["lod_levels"], count["lod_levels_behind"] = len(count.pop("levels")), len(count.pop("levels_behind"))
    out.update(count)
    return out


# the keys of a hit record that only a hit with a bounce has: NaN / False on a path's last segment, where `bounced` is False
_BOUNCE_VECTORS, _BOUNCE_SCALARS = ("ng", "ns", "dn"), ("u", "rho", "sn", "cs", "off")
_BOUNCE_FLAGS = ("smooth", "gone", "diffuse", "mirror", "glass")


def _path(O, cfg, pc, scene, rec, lights, cdf, sphere, mis, normals, nb, tex, frame_h, rng, d, count, albedo, seq_n, hits, smp, xs, ys):
    """one sample's paths from the camera along d [k, 3]: (R + terminal colour [k, 3], rng state [k], first hit id [k]).  albedo
    [k, 4]: the ALBEDO plane, None: not demodulated.  A new shading feature is a keyword of walk(), a block here marked with its
    name, and its counts in COUNTS"""
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
    cb = np.zeros(k, F32)                             # MIS: the cosine of the last diffuse bounce; read only where `sampled`
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
        acc[idx[lit][sbit[idx[lit]]]] = 0             # SPHERE: the hit before sampled the sphere, this hit's light is counted there
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
        again = sampled[j[emissive]]                  # NEE: the hit before sampled the lights
        if mis:                                       # MIS: this emission is one of two estimators, (T * Ke) * wb(g_hit)
            je = j[emissive][again]
            if len(je):
                eid = ids[hit][emissive][again]
                et = tris[eid.astype(np.int64) - 1]
                reached, inv_p = NM.hit_inv_p(lights, cdf, eid)
                gh = NM.g_hit(O, et[:, 0:3], et[:, 3:6], et[:, 6:9], oo[hit][emissive][again], dd[hit][emissive][again],
                              b1[hit][emissive][again], b2[hit][emissive][again], cb[je], inv_p)
                w_b = np.where(reached, NM.wb(gh), F32(1.0)).astype(F32)
                acc[je] = (acc[je] * w_b[:, None]).astype(F32)
                count["wb_min"] = min(count["wb_min"], float(w_b.min()))
                count["wb_max"] = max(count["wb_max"], float(w_b.max()))
        else:
            acc[j[emissive][again]] = 0               # ... this emission is counted there
        if seg > 0:
            count["dropped"] += int(again.sum())
            count["weighted"] += int(again.sum()) if mis else 0
            count["kept"] += int((~again).sum())
        alive[j[emissive]] = False
        keep = ~emissive
        j, m = j[keep], m[keep]
        hid = ids[hit][keep].astype(np.int64) - 1
        th, b1, b2, dd, oo = th[hit][keep], b1[hit][keep], b2[hit][keep], dd[hit][keep], oo[hit][keep]
        b0 = ((F32(1.0) - b1).astype(F32) - b2).astype(F32)                                          # :134
        tri = tris[hid]
        last = seg + 1 >= segments
        if tex is not None or not last:               # the stored normal: the texture's footprint and the bounce read it
            e1, e2 = (tri[:, 3:6] - tri[:, 0:3]).astype(F32), (tri[:, 6:9] - tri[:, 0:3]).astype(F32)
            n = normalize(O, _contract(O, "cross", e1, e2))                                          # :150
        alb = m[:, 0:3]
        lam, textured, mipped = np.zeros(len(j), F32), np.zeros(len(j), bool), np.zeros(len(j), bool)
        if tex is not None:                           # TEX
            texel, lam, textured, mipped = _texels(O, tex, hid % len(tex.tri_texture), b0, b1, b2, th, dot(O, n, dd), tri.reshape(-1, 3, 3),
                                                   spread0 if seg == 0 else MS.BOUNCE_SPREAD)
            alb = (alb * texel).astype(F32)
            count["mip_behind"] += int((mipped & glassed[j]).sum())
            if seg > 0:
                for key, sel in (("", mipped), ("_behind", mipped & glassed[j])):
                    count["levels" + key] |= set(np.floor(lam[sel]).astype(int).tolist())
                    count["lod_fraction" + key] += int((lam[sel] % 1 != 0).sum())
        if albedo is not None and seg == 0:           # DEMOD: into the plane, not into the throughput
            albedo[j, :3] = alb
        else:
            acc[j] = (acc[j] * alb).astype(F32)                                                      # :244
        record = None
        if hits is not None:
            record = dict(x=xs[j].copy(), y=ys[j].copy(), sample=np.full(len(j), smp), seg=np.full(len(j), seg), o=oo, d=dd, id=hid + 1,
                          b0=b0, b1=b1, b2=b2, lod=lam, albedo=alb, textured=textured, mipped=mipped, behind=glassed[j].copy())
        if last:                                      # the last segment: no light draw, no shadow query; the bounce's two draws
            rng[j] = _rng_next(O, _rng_next(O, rng[j])[0])[0]      # only move the stream (:256-257)
            if hits is not None:
                record.update(bounced=np.zeros(len(j), bool))
                record.update({key: np.full((len(j), 3), np.nan, F32) for key in _BOUNCE_VECTORS})
                record.update({key: np.full(len(j), np.nan, F32) for key in _BOUNCE_SCALARS})
                record.update({key: np.zeros(len(j), bool) for key in _BOUNCE_FLAGS})
                hits.append(record)
            break
        pos = fma(O, tri[:, 6:9], b2[:, None], fma(O, tri[:, 3:6], b1[:, None], (tri[:, 0:3] * b0[:, None]).astype(F32)))   # :137
        w = m[:, 3]
        glass = w > 0
        mirror = ~glass & (w.view(U32) != 0)
        diffuse = ~glass & ~mirror
        entering = dot(O, n, dd) < 0
        nf = np.where(entering[:, None], n, -n).astype(F32)                                          # :247: ng
        ns, smooth = hit_shading_normal(O, normals, hid, nb, b0, b1, b2, nf, dd)                     # NRM: ns is ng without normals
        if normals is not None:
            rs = np.asarray(normals.tri_smooth)[hid % nb] != 0
            count["smooth"] += int(smooth.sum())
            count["fallback4"] += int((rs & ~smooth).sum())
            count["fallback7"] += int((smooth & (ns == nf).all(1)).sum())
        q = np.flatnonzero(diffuse)
        jq = j[q]
        if L or sphere:
            x = fma(O, ray_offset, nf[q], pos[q])                                                     # :250, the bounce's origin (ng)
        tri_gain = None
        if L:                                         # NEE: the triangle sample, three draws, its gain added behind the sphere's
            r, u_l = _rng_next(O, rng[jq])
            r, u_a = _rng_next(O, r)
            r, u_b = _rng_next(O, r)
            rng[jq] = r
            if cdf is not None:                       # POWER: the weighted pick, and the inverse of its probability in the weight
                entry, inv_p = PW.pick_power(cdf, u_l)
                id1 = lights[entry]
                lt = tris[id1.astype(np.int64) - 1]
                wd, g, valid = PW.sample32_inv_p(O, lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, ns[q], u_a, u_b, inv_p)
            else:
                entry = N.pick(u_l, np.full(len(q), L))
                id1 = lights[entry]
                lt = tris[id1.astype(np.int64) - 1]
                s = N.sample32(O, N.cases_of(lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, ns[q], u_l, u_a, u_b, L))[:, :8].view(F32)
                wd, g, valid = s[:, 3:6], s[:, 6], s[:, 7] != 0
            if normals is not None:                   # NRM: the sample's side of ng
                side = ~smooth[q] | sample_side(O, wd, nf[q])
                count["side_invalid"] += int((valid & ~side).sum())
                valid = valid & side
            if mis:                                   # MIS: gm = g * m(g), one multiply behind the division
                g = NM.gm(g)
            count["picks"] += np.bincount(entry, minlength=L)
            ke = rec[(id1.astype(np.int64) - 1) % n_base, 4:7]
            with np.errstate(all="ignore"):
                gain = (((acc[jq] * ke).astype(F32)) * g[:, None]).astype(F32)                        # (T * Ke) * g
            seen, _, _, _ = closest_hits(O, tris, x[valid], wd[valid], tmax)
            reached = seen == id1[valid]
            tri_gain = (jq[valid][reached], gain[valid][reached])
            count["rays"] += int(valid.sum())
            count["samples"] += len(q)
            count["queries"] += int(valid.sum())
            count["lit"] += int(reached.sum())
            sampled[jq] = True                        # valid or not
            sampled[j[~diffuse]] = False              # a specular or dielectric hit clears the bit
        if sphere:                                    # SPHERE: two draws, no query, into R first; never weighed
            r, u_c = _rng_next(O, rng[jq])
            r, u_p = _rng_next(O, r)
            rng[jq] = r
            s = NS.sphere32(O, NS.cases_of(x, ns[q], light_c, r2, u_c, u_p)).view(F32)
            taken, valid = s[:, 4] != 0, s[:, 5] != 0
            if normals is not None:                   # NRM
                side = ~smooth[q] | sample_side(O, s[:, 0:3], nf[q])
                count["side_invalid"] += int((valid & ~side).sum())
                valid = valid & side
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
        dn = normalize(O, np.stack([fma(O, rho, cs, ns[:, 0]), fma(O, rho, sn, ns[:, 1]), (ns[:, 2] + u).astype(F32)], 1))   # :259-261 about ns
        if mis:                                       # MIS: the cosine the diffuse bounce leaves with, behind the normalize
            cb[jq] = dot(O, ns[q], dn[q])
        gone_side = np.zeros(len(j), bool)
        if normals is not None:                       # NRM: a diffuse d' behind ng
            gone_side[q] = smooth[q] & absorbed(O, dn[q], nf[q])
        if mirror.any():                              # specular.hpp: the lobe around the mirror direction
            nm, dm, gl = ns[mirror], dd[mirror], np.abs(w[mirror])
            c2 = (F32(-2.0) * dot(O, nm, dm)).astype(F32)
            refl = fma(O, c2[:, None], nm, dm)
            sph = np.stack([(rho[mirror] * cs[mirror]).astype(F32), (rho[mirror] * sn[mirror]).astype(F32), u[mirror]], 1)
            lobe = normalize(O, fma(O, gl[:, None], sph, refl))
            dn[mirror] = lobe
            lost = ~(dot(O, nm, lobe) > 0)
            if normals is not None:                   # NRM: a specular d' behind ng
                gone_side[mirror] = smooth[mirror] & absorbed(O, lobe, nf[mirror]) & ~lost
            gone = j[mirror][lost | gone_side[mirror]]
            acc[gone] = 0
            alive[gone] = False
        count["absorbed"] += int(gone_side.sum())
        acc[j[gone_side]] = 0
        alive[j[gone_side]] = False
        if glass.any():                               # dielectric.hpp, about ns with the side ng gave
            dg, transmitted = interface_faced(O, ns[glass], entering[glass], dd[glass], u1[glass], w[glass], m[glass, 4], m[glass, 5])
            dn[glass] = dg
            off[glass] = np.where(transmitted, -ray_offset, ray_offset).astype(F32)
            if normals is not None:                   # NRM: the side d' leaves on
                sided = dielectric_offset(O, dg, nf[glass], ray_offset)
                count["offset_changed"] += int((smooth[glass] & (sided != off[glass])).sum())
                off[glass] = np.where(smooth[glass], sided, off[glass])
            count["transmitted"] += int(transmitted.sum())
            count["reflected"] += int((~transmitted).sum())
            glassed[j[glass]] = True
        if hits is not None:
            record.update(bounced=np.ones(len(j), bool), ng=nf, ns=ns, dn=dn.copy(), u=u, rho=rho, sn=sn, cs=cs, off=off.copy(),
                          smooth=smooth, gone=gone_side.copy(), diffuse=diffuse, mirror=mirror, glass=glass)
            hits.append(record)
        o[j] = fma(O, off[:, None], nf, pos)                                                          # :250 (ng)
        d[j] = dn
    return (radiance + acc).astype(F32), rng, first_id                                                # R + terminal


def hit_table(hits):
    """the walker's hit records, one array per key over every shaded hit of the frame; the bounce's keys (ng, ns, dn, ...) hold NaN
    or False where `bounced` is False: the hit was its path's last segment"""
    return {k: np.concatenate([h[k] for h in hits]) for k in hits[0]} if hits else {}


# ------------------------------------------------------------------------------------------ the recording
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "walker_frames.npz")


@lru_cache(maxsize=None)
def _recording():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def recorded(group, *tag):
    """what one of the walkers this one replaced returned for the call `tag` of the group of calls `group` (a test and the walker it
    called; scripts/record_walker_frames.py wrote them at the commit the file names): IMAGE and HIT_ID, ALBEDO and seq_n where that
    walker had them, `picks` where it counted them, and its integer counts by name.  IMAGE may be held as the SHA-256 of its bytes
    (IMAGE_sha256).  A group or a tag the file does not hold is a KeyError: a failure, never a skip"""
    f, key = _recording(), ",".join(str(t) for t in tag)
    i = f[group + "/keys"].tolist().index(key) if group + "/keys" in f and key in f[group + "/keys"].tolist() else None
    if i is None:
        raise KeyError((group, key))
    out = {}
    for plane, dtype in (("IMAGE", F32), ("HIT_ID", U32), ("ALBEDO", F32), ("seq_n", np.int32), ("IMAGE_sha256", np.uint8)):
        if group + "/" + plane in f:
            out[plane] = f[group + "/" + plane][i].view(dtype)
    if group + "/picks" in f:
        ends = np.cumsum(f[group + "/picks_n"])
        out["picks"] = f[group + "/picks"][ends[i] - f[group + "/picks_n"][i]:ends[i]]
    out.update(zip(f[group + "/names"].tolist(), f[group + "/counts"][i].tolist()))
    return out


def same_image(got, want):
    """got's IMAGE is the recorded one bit for bit — by its bytes' SHA-256 where the recording holds only that"""
    if "IMAGE" in want:
        return np.array_equal(np.ascontiguousarray(got["IMAGE"]).view(U32), want["IMAGE"].view(U32))
    return hashlib.sha256(np.ascontiguousarray(got["IMAGE"], F32).tobytes()).digest() == want["IMAGE_sha256"].tobytes()
