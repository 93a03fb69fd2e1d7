#!/usr/bin/env python3
"""Regenerates tests/golden/obj_reader/expected.npz: what the six OBJ entry points of a GIVEN build of the library return
for every file of the corpus next to it (tests/obj_reader_calls.py lists what is kept: return codes, rtpt_last_error
texts, counts and every array, byte for byte).

    python tests/golden/make_obj_reader.py <path of librtpt_hip.so> [<commit it was built from>]

The expectations pin the readers' behaviour across a rewrite, so they are recorded from the library of the commit BEFORE the
rewrite, never from the code under test.  The entry points touch no device: no GPU is needed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]


def generate(lib_path):
    os.environ["RTPT_LIB_PATH"] = os.path.abspath(lib_path)  # read by abi when it is imported
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi
    import obj_reader_calls as R
    assert abi.LIB_PATH == os.path.abspath(lib_path)
    out = {}
    for name in R.corpus_files():
        for key, value in R.call_all(abi, os.path.join(R.CORPUS, name)).items():
            out[f"{name}/{key}"] = value
    return R.EXPECTED, out


if __name__ == "__main__":
    path, data = generate(sys.argv[1])
    data["recorded_at"] = np.str_(sys.argv[2] if len(sys.argv) > 2 else "")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", len(data), "arrays")
