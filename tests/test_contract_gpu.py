"""The numerics contract on the device, function by function and operand by operand: rtpt_selftest_contract (the functions the
frame kernels call, one thread per item) against oracle_contract_array on the operand classes of tests/contract_cases.py,
2^20 items per function in one launch, every output word.

Float words are equal bit for bit, the sign of a zero included; where BOTH are NaN the sign and payload are the processor's and
are not compared.  Integer and boolean words (f2i, the RNG states, reproject_pixel's pixel, ray_hits_light) are exact whatever
the operands, NaNs included.  tests/test_contract_cpu.py holds the oracle to exact rationals and to the known answers, and
asserts on the oracle alone that the items are not mostly NaN; this file repeats the known answers on the device.
rtpt_selftest_div mode 3 runs exact::div2_ against the compiler's two divisions over 2^33 operand triples of arbitrary bits."""
import numpy as np
import pytest

import contract_cases as CC
from test_contract_cpu import check_known, reproject_known

pytestmark = pytest.mark.gpu

N = 1 << 20


@pytest.fixture(scope="module")
def ctx(hip_lib):
    with hip_lib.Context(hip_lib.config_default(64, 48)) as c:
        yield c


def first_difference(fn, w, cls, got, want):
    """None, or a description of the first item whose output words differ under the rule of the module's docstring"""
    bad = got != want
    fo = list(CC.float_out_words(fn))
    if fo:
        both_nan = CC.is_nan_bits(got[:, fo]) & CC.is_nan_bits(want[:, fo])
        bad[:, fo] &= ~both_nan
    rows = np.nonzero(bad.any(1))[0]
    if not len(rows):
        return None
    i = int(rows[0])
    per_class = {CC.CLASSES[c]: int((cls[rows] == c).sum()) for c in np.unique(cls[rows])}
    return (f"{fn}: {len(rows)} of {len(w)} items differ ({per_class}); first: item {i} ({CC.CLASSES[cls[i]]}) "
            f"in {[f'{int(u):08x}' for u in w[i]]} device {[f'{int(u):08x}' for u in got[i]]} oracle {[f'{int(u):08x}' for u in want[i]]}")


@pytest.mark.parametrize("fn", CC.FNS)
def test_device_function_equals_the_oracle(ctx, oracle, fn):
    idx = CC.fn_index(fn)
    w, cls = CC.cases(fn, N)
    want = oracle.contract_array(idx, w)
    got = ctx.selftest_contract(idx, w)
    assert got.shape == want.shape == (N, CC.WORDS[idx][1])
    diff = first_difference(fn, w, cls, got, want)
    assert diff is None, diff


def test_known_answers_on_the_device(ctx):
    check_known(ctx.selftest_contract, "device")
    for w, want in reproject_known():
        got = ctx.selftest_contract(CC.fn_index("reproject_pixel"), w[None])[0]
        assert [int(g) for g in got] == want, ([hex(int(u)) for u in w], got, want)


def test_an_item_count_that_is_no_multiple_of_the_block(ctx, oracle):
    """257 and 1 items: the last block is partial and the words of the items behind it stay untouched"""
    for n in (1, 257):
        for fn in ("cross", "reproject_pixel"):
            w, _ = CC.cases(fn, 4096)
            w = w[np.random.default_rng(n).permutation(4096)[:n]]
            got, want = ctx.selftest_contract(CC.fn_index(fn), w), oracle.contract_array(CC.fn_index(fn), w)
            assert first_difference(fn, w, np.zeros(n, np.uint8), got, want) is None


def test_div2_on_the_device(ctx):
    """rtpt_selftest_div mode 3, one pass: 2^33 triples, b in a0's binade in every other one, a1 too in half of either kind"""
    bad, first = ctx.selftest_div(3, 0, 1)
    assert bad == 0, f"exact::div2_ differs from the compiler's divisions on {bad} quotients, e.g. numerator, b = {[hex(v) for v in first]}"


def test_refusals(ctx, hip_lib):
    w = np.zeros((4, 6), np.uint32)
    out = np.zeros((4, 1), np.uint32)
    for fn in (-1, len(CC.FNS)):
        with pytest.raises(hip_lib.RtptError):
            hip_lib._check(ctx._lib.rtpt_selftest_contract(ctx._h, fn, hip_lib._ptr(w), hip_lib._ptr(out), 4))
    with pytest.raises(hip_lib.RtptError):
        hip_lib._check(ctx._lib.rtpt_selftest_contract(ctx._h, 0, None, hip_lib._ptr(out), 4))
    with pytest.raises(ValueError):
        ctx.selftest_contract(0, np.zeros((4, 5), np.uint32))
    with pytest.raises(hip_lib.RtptError):
        ctx.selftest_div(4, 0, 1)
