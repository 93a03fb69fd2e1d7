"""The sphere sample of next-event estimation (RTPT_FLAG_EXT_NEE_SPHERE; csrc/light_sample.hpp states the rules and the
arithmetic) for test_nee_sphere_*.py: its numpy restatements, the records of a scene without a material table and the scenes.

sphere32 follows light::sphere_sample one float32 operation per device operation, through the pieces of dielectric_scenes (the
contract's dot, normalize, sincos2pi and fused multiply-add; numpy's square root, products and divisions, all correctly rounded):
it is what tests/test_nee_sphere_gpu.py holds the device function to, bit for bit.  sphere64 is the same in float64 from the
float32 operands as they are, the same orthonormal pair included (the direction depends on it).

tests/path_walker.py walks the paths (`sphere=`): two draws behind the triangle sample's three, the sphere's gain into R before the
triangle's, the sphere bit beside the sampled bit.  With sphere=False it takes no draw of the sphere's, which
tests/test_nee_sphere_cpu.py asks for bit by bit against the recorded frames of the walkers without it.  A scene without a material
table walks with normal_keyed_records."""
from functools import lru_cache

import numpy as np

import dielectric_scenes as DS
import nee_scenes as N
import pathtrace_scenes as P
from dielectric_scenes import _contract, dot, fma, normalize

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
