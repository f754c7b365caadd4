"""GPU: every output byte of mipnerf_preview_march and mipnerf_preview_mip_march on the cases of tests/preview_bytes_fixture.py against
tests/golden/preview_march_bytes.npz, which scripts/make_golden_preview_bytes.py recorded on the last tree whose two entry points had a
march kernel each (k_preview_march and k_preview_mip_march).  Both now launch the one kernel of csrc/preview_wave_march.hpp; this file
holds that kernel, and whatever is done to it later, to the bytes of the two it replaced -- on every ray, the degenerate ones included,
so arrays are compared as bytes, not as values."""
import os

import numpy as np
import pytest

import preview_bytes_fixture as bf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", bf.GOLDEN)) as z:
        return {k: z[k] for k in z.files}


def test_the_golden_file_holds_exactly_the_cases(golden):
    want = {f"{n}_{k}" for n in bf.case_names() for k in (bf.PLAIN_ARRAYS if n.startswith("plain") else bf.MIP_ARRAYS)}
    assert set(golden) == want and len(bf.case_names()) == 25


@pytest.mark.parametrize("name", bf.case_names())
def test_every_output_byte_is_the_recorded_one(golden, name):
    got = bf.run_case(name)
    assert (got["steps"] > 0).sum() > 100                    # the case marches: most rays evaluate samples
    for k in bf.PLAIN_ARRAYS if name.startswith("plain") else bf.MIP_ARRAYS:
        want = golden[f"{name}_{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k)
        assert got[k].tobytes() == want.tobytes(), (name, k, np.flatnonzero((got[k] != want).reshape(want.shape[0], -1).any(-1)))
