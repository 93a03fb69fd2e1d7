"""The numerics contract (oracle/det_math.h) pinned to the real functions: each deterministic
sequence must agree with double-precision libm to a few ulp over the ranges the path uses, so that
"bit-exact against the oracle" also means "a faithful sin/cos/log/exp"."""
import numpy as np


def ulp_err(got, want64):
    want32 = want64.astype(np.float32)
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    ulp = np.maximum(ulp, np.finfo(np.float32).tiny)
    return np.abs(got.astype(np.float64) - want64) / ulp


def test_log_accuracy(oracle):
    rng = np.random.default_rng(0)
    x = np.exp(rng.uniform(np.log(1e-38), 0.0, 400_000)).astype(np.float32)
    x = np.concatenate([x, np.float32([1.0, 0.5, 0.70710678, 2.0 ** -32, 1e-38, 1.17549435e-38])])
    got = oracle.math_array(0, x)
    err = ulp_err(got, np.log(x.astype(np.float64)))
    assert err.max() <= 2.0, err.max()
    assert oracle.math_array(0, np.float32([1.0]))[0] == 0.0


def test_log_accuracy_on_every_positive_finite_input(oracle):
    """dm_log states its domain as finite x > 0, and the frame uses (1e-38, 1] only.  Measured against float64 libm over 4 * 10^6
    positive finite patterns of arbitrary bits, six significands in each of the 255 exponent fields and 2 * 10^6 points of
    [0.7, 1.45]: 0.75 ulp at most (0.50 on the subnormals, 0.82 in the dense sample around 1): the file's 2-ulp bound holds on
    the whole domain."""
    rng = np.random.default_rng(4)
    b = rng.integers(1, 0x7f7fffff, 400_000, dtype=np.int64).astype(np.uint32)
    ex = ((np.arange(0, 255, dtype=np.uint32)[:, None] << 23) | np.array([0, 1, 0x3504f3, 0x3504f4, 0x400000, 0x7fffff], np.uint32)[None, :]).ravel()
    near1 = (np.float32(1) + rng.uniform(-0.3, 0.45, 100_000).astype(np.float32)).view(np.uint32)
    x = np.concatenate([b, ex[ex != 0], near1, np.uint32([1, 0x007fffff, 0x00800000, 0x7f7fffff, 0x3f7fffff, 0x3f800001])]).view(np.float32)
    assert x.min() == np.float32(2.0 ** -149) and x.max() == np.finfo(np.float32).max
    err = ulp_err(oracle.math_array(0, x), np.log(x.astype(np.float64)))
    assert err.max() <= 2.0, (err.max(), x[err.argmax()])


def test_sincos_accuracy(oracle):
    u = np.random.default_rng(1).uniform(0, 1, 400_000).astype(np.float32)
    u = np.concatenate([u, np.float32([0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0])])
    for op, fn in ((1, np.sin), (2, np.cos)):
        got = oracle.math_array(op, u).astype(np.float64)
        want = fn(2 * np.pi * u.astype(np.float64))
        # absolute error: GLSL allows 2^-11 on sin/cos; the contract is ~1e-7
        assert np.abs(got - want).max() < 2.5e-7
    s, c = oracle.math_array(1, u).astype(np.float64), oracle.math_array(2, u).astype(np.float64)
    assert np.abs(s * s + c * c - 1).max() < 5e-7
    assert oracle.math_array(1, np.float32([0.25]))[0] == 1.0 and oracle.math_array(2, np.float32([0.5]))[0] == -1.0


def test_exp_accuracy(oracle):
    x = np.random.default_rng(2).uniform(-87, 0, 400_000).astype(np.float32)
    got = oracle.math_array(5, x)
    err = ulp_err(got, np.exp(x.astype(np.float64)))
    assert err.max() <= 2.0, err.max()
    assert oracle.math_array(5, np.float32([0.0, -0.0]))[0] == 1.0
    assert oracle.math_array(5, np.float32([-100.0]))[0] == 0.0


def test_exp_accuracy_above_zero(oracle):
    """dm_exp takes the whole line (x > 88 is +inf) and the filter uses x <= 0 only.  Measured against float64 libm over 2 * 10^6
    uniform points of (0, 88] and the ends: 1.0006 ulp at most (at x = 26.73; 0.98 below 20, 0.97 above 60): the file's 2-ulp bound
    holds there too."""
    x = np.random.default_rng(5).uniform(0, 88, 400_000).astype(np.float32)
    x = np.concatenate([x[x > 0], np.float32([88.0, np.nextafter(np.float32(88), np.float32(0)), 2.0 ** -149, 1.0, 87.5, 2.0 ** -24])])
    got = oracle.math_array(5, x)
    assert np.isfinite(got).all()
    err = ulp_err(got, np.exp(x.astype(np.float64)))
    assert err.max() <= 2.0, (err.max(), x[err.argmax()])
    beyond = np.float32([np.nextafter(np.float32(88), np.float32(89)), 100.0, np.inf, np.nextafter(np.float32(-87), np.float32(-88)), -np.inf])
    assert oracle.math_array(5, beyond).tolist() == [np.inf, np.inf, np.inf, 0.0, 0.0]
    assert np.isnan(oracle.math_array(5, np.float32([np.nan]))[0])


def test_powi_and_f2i(oracle):
    lib = oracle.lib()
    for x in (0.0, 0.5, 0.999, 1.0, 0.99999994):
        want = np.float32(x)
        for _ in range(7):
            want = np.float32(want * want)          # 128 = 2^7: seven squarings
        assert np.float32(lib.oracle_powi(np.float32(x), 128)) == want
    assert lib.oracle_powi(np.float32(3.0), 5) == 243.0 and lib.oracle_powi(np.float32(3.0), 1) == 3.0
    # f2i is GLSL's ivec2(vec2): truncation toward zero; the contract adds NaN -> 0 and saturation (v_cvt_i32_f32)
    f2i = lambda x: oracle.contract_array(oracle.CONTRACT_FNS.index("f2i"), np.float32(x).view(np.uint32)[:, None])[:, 0].view(np.int32)  # noqa: E731
    x = np.float32([0.0, -0.0, 0.5, -0.5, 0.99999994, -0.99999994, 1.0, -1.0, 1.5, -1.5, 2.5, -2.5, 3839.9998, 16777216.0, -16777216.0, 2147483520.0,
                    -2147483520.0, 2.0 ** 31, -2.0 ** 31, 2147483904.0, -2147483904.0, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan, 2.0 ** -149])
    want = [0, 0, 0, 0, 0, 0, 1, -1, 1, -1, 2, -2, 3839, 16777216, -16777216, 2147483520, -2147483520, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31,
            2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0, 0]
    assert f2i(x).tolist() == want
    assert f2i(np.uint32([0xffc00000, 0x7f800001, 0xffffffff]).view(np.float32)).tolist() == [0, 0, 0], "every NaN, either sign"
    y = (np.random.default_rng(6).uniform(-1, 1, 100_000) * 2.0 ** 31).astype(np.float32)
    y = y[np.abs(y) < 2.0 ** 31]
    assert np.array_equal(f2i(y).astype(np.int64), np.trunc(y.astype(np.float64)).astype(np.int64))


def test_sqrt_rcp_are_ieee(oracle):
    x = np.random.default_rng(3).uniform(1e-6, 1e6, 200_000).astype(np.float32)
    assert np.array_equal(oracle.math_array(3, x), np.sqrt(x))
    assert np.array_equal(oracle.math_array(4, x), (np.float32(1.0) / x).astype(np.float32))
