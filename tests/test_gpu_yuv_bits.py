"""GPU: the bit pin of the YUV kernels — binyuv_to_frame, binyuv_from_frame, binrate_blend_to_yuv and binclip_yuv_to_bgr return, on
every case of tests/yuv_bit_cases.py (rounding ties, NaN and infinities included, both data paths, blocks that stride unevenly), bit
for bit what tests/golden/make_yuv_bits.py recorded from the commit named in tests/golden/yuv_bits.json: the load, store and launch
stages may move between files, the bytes may not.  CPU side: test_cpu_yuv_bit_cases.py."""
import json
import os

import pytest

import yuv_bit_cases as YB
from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(REPO, "tests", "golden", "yuv_bits.json")) as f:
        rec = json.load(f)
    assert rec["left_out"] == [], "the fixture leaves cases out: it pins less than the table"
    assert sorted(rec["bits"]) == sorted(YB.KEYS), "tests/golden/yuv_bits.json and tests/yuv_bit_cases.py name different cases"
    return rec


@pytest.mark.parametrize("key", YB.KEYS)
def test_yuv_bits_are_the_recorded_ones(key, recorded):
    got, want = YB.digests(key), recorded["bits"][key]
    assert sorted(got) == sorted(want), key
    differ = [name for name in got if got[name] != want[name]]
    assert not differ, f"{key}: {len(differ)} of {len(got)} buffers differ from commit {recorded['recorded_from']}: {differ[:4]}"
