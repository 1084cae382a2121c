"""The CPU half of the top-of-the-domain tests (tests/domain_top_cases.py): the case table's conditions, computed without a GPU, and
the method itself at a scaled-down geometry with float32 torch as the stand-in kernel: the right restatement passes bit for bit and
each deliberately wrong one (domain_top_cases.WRONG) is reported.  The census counts are held to a brute-force count."""
import numpy as np
import pytest
import torch

import abi_cases
import conv_ref_cases as rc
import domain_top_cases as dt
import poison

CPU = torch.device("cpu")
CASE_SHAPES = [(c.tag, s) for c in dt.CASES for s in dt.shapes(c)]


def _families(nterms):
    return ("A", "B") if nterms == 3 else ("A",)


def _out_plane(case, shape):
    n, h, w = shape
    s = dt.row_scale(case)
    return (n, int(h * s), int(w * s))


@pytest.mark.parametrize("tag,shape", CASE_SHAPES)
def test_table_conditions(tag, shape):
    """Conditions 1, 3 and 5 of the table, and that the shape IS the top: accepted, and its largest plane within 2^16 pixels of 2^26."""
    case = dt.BY_TAG[tag]
    n, h, w = shape
    assert dt.NHW_LIMIT == abi_cases.NHW_LIMIT
    on, oh, ow = _out_plane(case, shape)
    largest = max(n * h * w, on * oh * ow if case.opts.get("epilogue") != "subpix" else 0)     # fp32 NCHW stores have no plane
    assert n * h * w < dt.NHW_LIMIT and dt.NHW_LIMIT - (1 << 16) <= largest < dt.NHW_LIMIT, (shape, largest)
    if case.opts.get("y_unshuf") or case.opts.get("epilogue") == "subpix":
        assert h % 2 == 0 and w % 2 == 0 or not case.opts.get("y_unshuf")
    assert dt.wrap_is_visible(w) and dt.wrap_is_visible(ow), "a power-of-two shift is a whole number of periods"
    assert dt.P % 2 == 1 and all(dt.P % t for t in (2, 8, 16))
    assert dt.phases_differ(n)
    assert dt.out_period(case)[0] * 4 < oh, "fewer than four periods"
    for nterms in dt.NTERMS:
        live = dt.live_bytes(case, nterms, shape)
        print(f"[domain-top] table case={tag} nterms={nterms} shape={rc.shape_str(shape)} live={live / 2 ** 30:.2f} GiB")
        assert live <= dt.MAX_LIVE_BYTES, (tag, nterms, shape, live)


@pytest.mark.parametrize("tag", dt.TAGS)
def test_exactness_conditions(tag):
    """Condition 2.  The analytic form holds for the periods of every shape; conv_ref_cases.conditions() itself, evaluated, holds on
    every band of the narrowest shape (the same draw rule, 70 or 35 columns)."""
    case = dt.BY_TAG[tag]
    for shape in dt.shapes(case):
        for family in ("A", "B"):
            opnd = dt.period_operands(tag, family, shape[2])
            assert dt.sufficient_conditions(case, family, opnd) == []
    shape = dt.shapes(case)[1]
    for family in ("A", "B"):
        opnd = dt.period_operands(tag, family, shape[2])
        for (img, r0, r1, _, _) in dt.bands_of(case, shape):
            bo = dt.band_operands(case, opnd, img, r0, r1, CPU)
            for nterms in ((3, 1) if family == "A" else (3,)):
                assert rc.conditions(case, nterms, family, bo) == [], (tag, family, nterms, img, r0)


def _run(tag, nterms, family, shape, wrong=None):
    case = dt.BY_TAG[tag]
    small = dt.SCALED_DOWN[shape]
    opnd = dt.period_operands(tag, family, small[2])
    with poison.poisoned(0x47, devices=("cpu",)) as rec:
        dev_in = dt.expand_operands(case, nterms, small, opnd, CPU)
        outs = dt.stand_in(case, nterms, small, opnd, dev_in, wrong)
        if outs is None:
            return None
        rec.check_guards()
        return dt.check_outputs(case, nterms, family, small, opnd, outs, CPU, label="stand-in")


@pytest.mark.parametrize("nterms", dt.NTERMS)
@pytest.mark.parametrize("tag,shape", CASE_SHAPES)
def test_the_right_restatement_passes_every_row(tag, shape, nterms):
    for family in _families(nterms):
        res = _run(tag, nterms, family, shape)
        assert res["rows"] > 0


WRONG_CASES = (("p3", 1, "A"), ("p5", 3, "B"), ("s3", 3, "A"), ("f5_subpix", 1, "A"), ("b3_unshuf", 3, "B"), ("tail_o3", 3, "A"))


@pytest.mark.parametrize("wrong", dt.WRONG)
@pytest.mark.parametrize("tag,nterms,family", WRONG_CASES)
def test_a_wrong_restatement_is_reported(tag, nterms, family, wrong):
    caught = 0
    for shape in dt.shapes(dt.BY_TAG[tag]):
        if wrong == "image_1_reads_image_0" and shape[0] == 1:
            continue
        with pytest.raises(AssertionError, match="elements differ"):       # the element mismatch itself, no other assertion
            _run(tag, nterms, family, shape, wrong)
        caught += 1
    assert caught or wrong == "image_1_reads_image_0"


def test_one_image_read_for_another_has_a_case_with_several_images():
    assert any(s[0] > 1 for t, _, _ in WRONG_CASES for s in dt.shapes(dt.BY_TAG[t]))


@pytest.mark.parametrize("ks", dt.WGRAD_KS)
def test_census_counts_match_a_brute_force_count(ks):
    for shape in ((3, 7, 9), (1, 13, 6), (2, 5, 4), (1, 1, 1), (2, 3, 1)):
        assert np.array_equal(dt.census_counts(shape, ks), dt.census_brute(shape, ks)), (shape, ks)
    for shape in (dt.WIDE, dt.TALL):
        counts = dt.census_counts(shape, ks)
        # at most 2^24 (the centre tap of the wide shape is exactly ceil((2^26 - 1) / 4) = 2^24): every partial sum is an fp32 integer
        assert counts.max() <= (1 << 24) and counts.min() > (1 << 23), (shape, ks, counts)


def test_the_band_reference_is_the_suites_weight_gradient():
    import wgrad_cases as wg
    gen = torch.Generator().manual_seed(3)
    for ks in dt.WGRAD_KS:
        x = torch.randint(-3, 4, (2, 5, 7, 9), generator=gen).float()
        g = torch.randint(-3, 4, (2, 4, 7, 9), generator=gen).float()
        for a, b in zip(dt.wgrad_ref(x, g, ks), wg.reference(x, g, ks)):
            assert torch.equal(a, b), ks
        xb, gb = x + 2.0 ** -11, g - 2.0 ** -11
        hs = [wg.split16(t) for t in (xb, gb)]
        for a, b in zip(dt.wgrad_split_ref(xb, gb, ks, 3), wg.split_reference(hs[0][0], hs[0][1], hs[1][0], hs[1][1], ks, 3)):
            assert torch.equal(a, b), ks


def test_bands_sit_where_the_offsets_change():
    for shape in (dt.WIDE, dt.TALL):
        n, h, w = shape
        runs = dt.band_starts(shape)
        rows = {r for a, b in runs for r in range(a, b)}
        assert all(a // h == (b - 1) // h for a, b in runs), "a run crosses an image"
        assert 0 in rows and n * h - 1 in rows
        for k in (28, 29, 30):
            row = ((1 << k) // 32) // w
            assert row in rows and row - 1 in rows and row + 1 in rows, (shape, k)
        assert min(((1 << 31) // 32 - 1) // w, n * h - 1) in rows
        assert len(rows) <= 6 * dt.BAND_ROWS


@pytest.mark.parametrize("ks", dt.WGRAD_KS)
def test_band_values_keep_the_exactness_condition(ks):
    """The bands of the tall shape (the wide one's are evaluated by the GPU module, which asserts the same bound)."""
    for family, nterms in (("A", 1), ("A", 3), ("B", 3)):
        runs, data, dw, db, bound = dt.band_reference(dt.TALL, ks, family, nterms)
        assert bound * (1.0 if family == "A" else 2.0 ** 11) < rc.EXACT_LIMIT
        assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0
        assert torch.equal(dw.float().double(), dw) and torch.equal(db.float().double(), db)
    assert dt.wgrad_live_bytes(dt.WIDE, ks, 3)[0] <= dt.MAX_LIVE_BYTES and dt.wgrad_live_bytes(dt.WIDE, ks, 3)[1] < (10 << 20)


def test_layout_launch_limit_is_the_tables():
    assert abi_cases.LAYOUT_MAX_THREADS == (1 << 32) - 256
    n, h, w = dt.WIDE
    assert 31 * n * h * w * 2 <= abi_cases.LAYOUT_MAX_THREADS < 32 * n * h * w * 2
    assert 63 * n * h * w <= abi_cases.LAYOUT_MAX_THREADS < 64 * n * h * w


def test_the_convlstm_sum_decomposition_is_the_whole_tensors_gradient():
    """dw, db of the periodic tensor from the batch of three-row images equal float64 autograd over the whole (small) tensor; and the
    whole comparison passes float32 torch as the stand-in kernel."""
    shape = (2, 95, 9)
    per = dt.lstm_period(shape[2])
    full = dt.lstm_expand(per, shape, CPU)
    full["w"], full["b"] = per["w"], per["b"]
    r64 = dt.lstm_eval(full, torch.float64)
    batch, rw = dt.lstm_sum_batch(per, shape, CPU)
    s64 = dt.lstm_eval(batch, torch.float64, rw)
    for nm in ("dw", "db"):
        assert float((s64[nm] - r64[nm]).abs().max()) <= 1e-12 * float(r64[nm].abs().max()), nm
    got = dt.lstm_eval(full, torch.float32)
    dt.lstm_check(shape, per, got, CPU, CPU, label="stand-in")
    late = dict(got, h=torch.cat((got["h"][:, :, :1], got["h"][:, :, :-1]), 2))
    with pytest.raises(AssertionError):
        dt.lstm_check(shape, per, late, CPU, CPU, label="one row late")
    other = dict(got, gx=got["gx"][[0, 0]])
    with pytest.raises(AssertionError):
        dt.lstm_check(shape, per, other, CPU, CPU, label="image 0 for image 1")


def test_the_plan_comparison_passes_float32_torch_and_reports_a_late_row():
    from bin_amd.weights import general_rdn_weights
    from oracle import rdn_oracle as O
    from rdn_config_cases import FWD_BARS
    shape = (2, 190, 12)
    weights = general_rdn_weights(0, dt.PLAN_K, dt.PLAN_CFG)
    pers = dt.plan_periods(shape[2])
    frames = dt.plan_frames(pers, shape, CPU)
    with torch.no_grad():
        y = O.rdn(frames, {f"m.{nm}": torch.from_numpy(v) for nm, v in weights.items()}, "m")
    dt.plan_check(shape, pers, weights, y, CPU, CPU, FWD_BARS["f16x3"], label="float32 torch")
    late = torch.cat((y[:, :, :1], y[:, :, :-1]), 2)
    with pytest.raises(AssertionError):
        dt.plan_check(shape, pers, weights, late, CPU, CPU, FWD_BARS["f16"], label="one row late")
    with pytest.raises(AssertionError):
        dt.plan_check(shape, pers, weights, y[[1, 0]], CPU, CPU, FWD_BARS["f16"], label="images swapped")
    n, h, w = dt.PLAN_SHAPE
    from bin_amd import _lib as L
    s = L.BinRdnShape()
    s.G0, s.D, s.C, s.G = dt.PLAN_CFG
    for nterms in (1, 3):
        ws = L.lib().binhip_rdn_workspace_bytes(n, h, w, dt.PLAN_K, nterms, s)
        live = ws + (dt.PLAN_K + 1) * n * 3 * h * w * 4
        print(f"[domain-top] table case=plan nterms={nterms} workspace={ws / 2 ** 30:.2f} GiB live={live / 2 ** 30:.2f} GiB")
        assert 0 < ws and live <= dt.MAX_LIVE_BYTES


def test_the_gsub_comparison_passes_the_definition_and_reports_a_live_ring():
    """gsub_check against the kernel's definition restated on the whole (small) tensor: pixel-unshuffle of the scaled gradient with
    the outermost ring zeroed.  Without the zeroing, or one image for another, it must report."""
    import torch.nn.functional as F
    shape, scale = (2, 160, 12), 4096.0
    n, h, w = shape
    per = dt.gsub_period(w)
    g = dt.expand_rows(per, n, h, 2 * dt.P, lambda i: dt.PHASES[i]).permute(1, 0, 2, 3).contiguous()

    def planes(g, ring=True):
        g = g * scale
        if ring:
            g = g.clone()
            g[:, :, 0, :] = g[:, :, -1, :] = 0
            g[:, :, :, 0] = g[:, :, :, -1] = 0
        return dt.split_planes(F.pixel_unshuffle(g, 2), 3)
    hi, lo = planes(g)
    assert float(lo.abs().max()) > 0 and not bool(hi[..., 12:].any())
    dt.gsub_check(shape, per, scale, hi, lo, label="definition")
    dt.gsub_check(shape, per, scale, hi, None, label="definition, hi alone")
    for label, (bh, bl) in (("ring kept", planes(g, ring=False)), ("images swapped", planes(g[[1, 0]]))):
        with pytest.raises(AssertionError, match="elements differ"):
            dt.gsub_check(shape, per, scale, bh, bl, label=label)
