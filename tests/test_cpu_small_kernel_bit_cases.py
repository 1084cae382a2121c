"""The case table of the small-kernel bit pin (tests/small_kernel_bit_cases.py) and its fixture (tests/golden/small_kernel_bits.json)
name the same cases, the fixture holds a digest for every output buffer of every call, and it stays a small file."""
import json
import os

import loss_cases as LS
import small_kernel_bit_cases as bc
from conftest import REPO

FIXTURE = os.path.join(REPO, "tests", "golden", "small_kernel_bits.json")
SIZE_LIMIT = 1 << 20                                        # no committed file may be larger than 1 MiB


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_and_case_table_name_the_same_cases():
    rec = _fixture()
    assert rec["left_out"] == []
    assert sorted(rec["bits"]) == sorted(bc.KEYS) and len(set(bc.KEYS)) == len(bc.KEYS)


def test_fixture_stays_under_the_committed_file_size_limit():
    assert os.path.getsize(FIXTURE) < SIZE_LIMIT


def test_every_output_buffer_has_a_digest():
    for key, got in _fixture()["bits"].items():
        parts = key.split("/")
        if parts[0] == "lstm":
            want = set(bc.lstm_buffers(key))
        elif parts[0] == "gates":
            want = {"c", "h", "dgates"} | ({"g_cprev"} if parts[2] == "cp" else set())
        elif parts[0] == "ploss":
            want = {"loss", "partials", "gx_only", "gy_only", "gx_both", "gy_both"}
        elif parts[0] == "charb":
            want = {"loss", "partials", "gx_both", "gy_both"}
        elif parts[0] == "mloss":
            _, idx = LS.multi_pairs(int(parts[2][1:]), list(range(34)))
            want = {"loss", "terms", "partials"} | {f"g{i}" for i in bc.multi_where(idx)}
        else:
            assert parts[0] == "gscale", key
            want = {"scale", "partials"}
        assert set(got) == want, key
        assert all(len(v) == 64 for v in got.values())


def test_the_multi_term_backward_cases_hold_a_tensor_in_two_terms_and_a_negative_sign():
    for T in LS.MULTI_T[1:]:
        _, idx = LS.multi_pairs(T, list(range(34)))
        where = bc.multi_where(idx).values()
        assert any(len(w) == 2 for w in where) and any(s < 0 for w in where for _, s in w)
