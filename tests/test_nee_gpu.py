"""The light sample of next-event estimation on the device (csrc/light_sample.hpp, k_selftest_light_sample): the function the
tracing kernels are to call, against its numpy restatement (tests/nee_scenes.py, held to float64 and to Lambert's closed form on
the CPU, tests/test_nee_cpu.py), bit for bit.  Fails on a library without rtpt_selftest_light_sample."""
import numpy as np
import pytest

import nee_scenes as N
import pathtrace_scenes as P
import test_pathtrace_scenes_gpu as T
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32


def test_light_sample_equals_the_restatement(hip_lib, oracle):
    """rtpt_selftest_light_sample, one case per lane, against nee_scenes.sample32 bit for bit: y, wd, g, the validity and the pick,
    on the hostile cases (a light without area, x on the light's plane and behind the surface, u_a on 0 and next to 1, u_l next
    to 1 with 1, 3 and 2^24 entries, r2 at the smallest normal and at 0) and on 4,096 seeded ones"""
    abi = hip_lib
    cases = np.concatenate([N.hostile_cases(), N.seeded_cases()[0]])
    scene = P.closed_room("small")
    with abi.Context(T._config(abi, scene, 64, 12, 1, 1, 0)) as ctx:
        got = ctx.selftest_light_sample(cases)
    want = N.sample32(oracle, cases)
    same_bits(got[:, 0:3].view(F32), want[:, 0:3].view(F32), ("light_sample", "y"))
    same_bits(got[:, 3:6].view(F32), want[:, 3:6].view(F32), ("light_sample", "wd"))
    same_bits(got[:, 6].view(F32), want[:, 6].view(F32), ("light_sample", "g"))
    same_bits(got[:, 7].view(F32), want[:, 7].view(F32), ("light_sample", "valid"))
    assert np.array_equal(got[:, 8], want[:, 8]), "the pick"
