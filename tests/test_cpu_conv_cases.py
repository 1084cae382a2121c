"""The case table of the forward-kernel bit pin (tests/conv_cases.py) and its fixture (tests/golden/conv_bits.json) name the same cases,
and the fixture holds a digest for every output buffer of every call."""
import json
import os

import conv_cases as cc
from conftest import REPO


def _fixture():
    with open(os.path.join(REPO, "tests", "golden", "conv_bits.json")) as f:
        return json.load(f)


def test_fixture_and_case_table_name_the_same_cases():
    rec = _fixture()
    assert rec["left_out"] == []
    assert sorted(rec["bits"]) == sorted(cc.KEYS) and len(set(cc.KEYS)) == len(cc.KEYS)
    assert all(set(c.rows) == set(cc.NTERMS) for c in cc.CASES)


def test_every_output_buffer_has_a_digest():
    for key, got in _fixture()["bits"].items():
        case, nterms, shape = cc.parse_key(key)
        assert shape in cc.shapes(case)
        if case.opts.get("epilogue") in ("final", "subpix"):
            want = {"f32"}
        else:
            want = {"hi"} | ({"lo"} if nterms == 3 else set())
            if case.opts.get("store_o3"):
                want |= {"o3_" + b for b in want}
        assert set(got) == want, key
        assert all(len(v) == 64 for v in got.values())
