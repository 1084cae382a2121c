"""The case table of the YUV kernels' bit pin (tests/yuv_bit_cases.py) and its fixture (tests/golden/yuv_bits.json) name the same
cases, the fixture holds a digest for every output buffer, and the strided cases stride the way they are meant to."""
import json
import os

import video_cases as VC
import yuv_bit_cases as YB
from conftest import REPO


def _fixture():
    with open(os.path.join(REPO, "tests", "golden", "yuv_bits.json")) as f:
        return json.load(f)


def test_fixture_and_case_table_name_the_same_cases():
    rec = _fixture()
    assert rec["left_out"] == []
    assert len(rec["recorded_from"]) >= 7
    assert sorted(rec["bits"]) == sorted(YB.KEYS) and len(set(YB.KEYS)) == len(YB.KEYS)
    assert len(YB.KEYS) == len(YB.OPS) * (len(VC.CASES) * len(VC.MATRIX_RANGE) + 1)


def test_every_output_buffer_has_a_digest():
    for key, got in _fixture()["bits"].items():
        names = [name for name, _ in YB.subcases(key)]
        assert len(set(names)) == len(names) and set(got) == set(names), key
        assert all(len(v) == 64 for v in got.values())
        assert {name.rsplit("/", 1)[1] for name in names} == {"off0", "off1"}, "both data paths"


def test_table_covers_what_the_issue_of_the_pin_names():
    subs = lambda op, case="6x10_420/bt601_full": [p for _, p in YB.subcases(f"{op}/{case}")]
    assert {p[0] for p in subs("to_frame")} == set(VC.pads_of(6, 10))
    assert {p[0] for p in subs("from_frame")} == {p[0] for p in subs("blend")} == set(VC.crops_of(6, 10))
    assert {p[1] for p in subs("blend")} == {0.0, 0.25, 0.6}
    assert YB.BGR_FRAMES == 3 and YB.bgr_stride("plus5", 90) == 95 and {p[1] for p in subs("to_bgr")} >= {"plus5"}


def test_strided_cases_make_lanes_loop_two_and_three_times():
    for op in YB.OPS:
        assert 2 * YB.STRIDE_LANES < YB.strided_items(op) < 3 * YB.STRIDE_LANES, op
        assert YB.parse_key(f"{op}/strided")[-1] is True
    n, h, w, chroma = YB.STRIDED_CLIP
    assert w % 4 == 0 and YB.bgr_stride("round16", VC.frame_bytes(h, w, chroma)) % 4 == 0, "the dword path strides too"
    assert YB.STRIDED_FRAME[1] % 4 == 0
