"""tests/conv_ref_cases.py without a GPU: the conditions of the exact operand families hold on the reference alone for every case, shape
and family; float32 torch, standing in for the kernel, passes the white-noise comparison (its e32 and bar are printed); and each of a
list of deliberately wrong restatements of the operation is caught by the comparison on at least one (case, family, shape) of the
table — which is how the suite shows that tests/test_gpu_conv_float64.py would notice a kernel that is wrong in that way."""
import pytest
import torch

import conv_cases as cc
import conv_ref_cases as rc


@pytest.mark.parametrize("tag", cc.TAGS)
def test_exact_family_conditions_hold(tag):
    case = cc.BY_TAG[tag]
    for shape in cc.shapes(case):
        for nterms in cc.NTERMS:
            for family in rc.families(nterms):
                if family == "C":
                    continue
                opnd = rc.operands(tag, family, shape)
                assert rc.conditions(case, nterms, family, opnd) == [], (tag, nterms, family, shape)
                # the probes are not trivial: the reference is not all zero, and family B keeps all three products live
                ref, _ = rc.references(tag, nterms, family, shape)
                assert all(bool(v.any()) for v in ref.values()) or shape == (1, 1, 1) or shape == (1, 2, 2), (tag, family, shape)
                if family == "B":
                    R = rc.as_read(opnd, 3)
                    for k, v in R.items():
                        if isinstance(v, tuple) and k != "mask":
                            assert bool(v[0].any()) and bool(v[1].any()), (tag, k, "a plane of family B is empty")


@pytest.mark.parametrize("tag", cc.TAGS)
def test_the_exact_families_pin_a_float64_restatement_bit_for_bit(tag):
    """The comparison code on its own reference: float64 torch restated with the plane stores passes A and B with ratio 0."""
    case = cc.BY_TAG[tag]
    for shape in cc.shapes(case):
        for nterms in cc.NTERMS:
            for family in rc.families(nterms)[:-1]:
                res = rc.compare(case, nterms, family, shape, rc.restated(case, nterms, family, shape), label="float64")
                assert all(r[3] == 0.0 for r in res.values())


@pytest.mark.parametrize("tag", cc.TAGS)
def test_float32_torch_passes_the_white_noise_bars(tag):
    case = cc.BY_TAG[tag]
    for shape in cc.shapes(case):
        for nterms in cc.NTERMS:
            rc.compare(case, nterms, "C", shape, rc.restated(case, nterms, "C", shape, dt=torch.float32), label="float32")


def test_pad_lane_table_names_the_cases_that_have_pad_lanes():
    """Outputs that end inside a chunk: backward-data cases whose cin is no multiple of 16 (forward plane cases all end on a chunk;
    FINAL outputs are fp32 NCHW of cout channels).  Each has its promise in PAD_LANES, and the reference really covers those lanes."""
    ragged = {c.tag for c in cc.CASES if c.kind == "bwd" and c.cin % 16 and not c.opts.get("y_unshuf")}
    assert ragged == set(rc.PAD_LANES)
    assert all(c.cout % 16 == 0 for c in cc.CASES if c.kind == "fwd" and c.opts.get("epilogue", "planes") == "planes")
    assert all((c.cout // 4) % 16 == 0 for c in cc.CASES if c.opts.get("epilogue") == "shuffle")
    for tag, promise in rc.PAD_LANES.items():
        assert promise == "acc"
        case = cc.BY_TAG[tag]
        for family in ("A", "C"):
            shape = cc.shapes(case)[1]
            ref, _ = rc.references(tag, 3, family, shape)
            acc = rc.as_read(rc.operands(tag, family, shape), 3)["acc"]
            assert ref["y"].shape[1] == cc.chunks(case.cin) * 16
            assert torch.equal(ref["y"][:, case.cin:], (acc[0] + acc[1])[:, case.cin:]) and bool(ref["y"][:, case.cin:].any())


def test_mask_probe_has_zeros_of_both_signs():
    for tag in ("b3_mask", "b1_lffd"):
        case = cc.BY_TAG[tag]
        m = rc.operands(tag, "A", cc.shapes(case)[2])["mask"][:, 16 * case.opts["mask_from"]:]
        assert bool(((m == 0) & ~torch.signbit(m)).any()) and bool(((m == 0) & torch.signbit(m)).any())


def _applies(wrong, case, family, shape):
    o, (n, h, w) = case.opts, shape
    return {
        "right_pad": case.ks > 1 and h > 1,
        "corner_tap_row16": case.ks > 1 and h > 16,
        "drop_wlo_xhi": family == "B",
        "mask_from_plus_1": "mask_from" in o,
        "mask_lt": "mask_from" in o,
        "res_extra_chunk": o.get("res_chunks", 0) > 0,
        "subpixel_swapped": o.get("epilogue") in ("shuffle", "subpix"),
        "gap_as_data": bool(o.get("x_cpg")),
        "mean_count": o.get("epilogue") in ("final", "subpix"),
        "second_image_from_first": n > 1,
    }[wrong]


@pytest.mark.parametrize("wrong", rc.WRONG)
def test_a_wrong_restatement_is_caught(wrong):
    """Per precision: at least one (case, family, shape) of the table where the wrong restatement applies fails the comparison; and
    every exact probe (A, B) it applies to fails, so the catch does not hang on one lucky case."""
    for nterms in cc.NTERMS:
        if wrong == "drop_wlo_xhi" and nterms == 1:
            continue
        caught, tried = [], 0
        for case in cc.CASES:
            for shape in cc.shapes(case):
                for family in rc.families(nterms):
                    if not _applies(wrong, case, family, shape):
                        continue
                    if family == "C" and (caught or wrong == "mask_lt"):      # white noise has no exact zeros; one C catch is enough
                        continue
                    tried += 1
                    try:
                        rc.compare(case, nterms, family, shape, rc.restated(case, nterms, family, shape, wrong=wrong), label=wrong)
                    except AssertionError:
                        caught.append((case.tag, family, shape))
                    else:
                        assert family == "C", f"{wrong}: the exact probe {case.tag} {family} {shape} nterms {nterms} did not notice"
                if len(caught) >= 6:
                    break
            if len(caught) >= 6:
                break
        assert caught, f"{wrong}: none of {tried} comparisons at nterms {nterms} failed"
        print(f"[conv-f64] wrong={wrong} nterms={nterms}: caught by {caught}")
