"""-m gpu: every reachable row of bh_dispatch_conv and the fused dense-block tail (tests/conv_cases.py), at both precisions and the
table's three front-end shapes, against float64 on the operands as the kernel reads them (tests/conv_ref_cases.py): integer and
split-exact probes that must match bit for bit, and the bit pin's own white noise within derived bars.  One line per comparison:
    [conv-f64] row=<dispatcher row> case= nterms= family= shape= out= e32= bar= kernel=<error> ratio=
tests/test_cpu_conv_ref_cases.py shows that the same comparison catches a kernel that is wrong in any of ten ways."""
import pytest
import torch

import conv_cases as cc
import conv_ref_cases as rc

pytestmark = pytest.mark.gpu


def _check_uploaded(tag, nterms, opnd, inputs):
    """The planes the kernel reads are the split the reference assumes, bit for bit (values: +0 and -0 are one stored value)."""
    R = rc.as_read(opnd, nterms)
    for name, cp in inputs.items():
        if cp is None:
            continue
        c = R[name][0].shape[1]
        assert torch.equal(rc.planes_to_nchw(cp.hi)[:, :c], R[name][0]), (tag, name, "hi")
        assert not bool(rc.planes_to_nchw(cp.hi)[:, c:].any()), (tag, name, "channel padding")
        if nterms == 3:
            assert torch.equal(rc.planes_to_nchw(cp.lo)[:, :c], R[name][1]), (tag, name, "lo")


def _decoded(outs):
    return {nm: v.double().cpu() if nm == "f32" else rc.decode(v) for nm, v in outs.items()}


def test_the_fp32_class_bar_is_the_suites():
    import test_gpu_conv
    assert rc.B_F32 <= test_gpu_conv.TOL_OPS[3]


@pytest.mark.parametrize("nterms", cc.NTERMS)
@pytest.mark.parametrize("tag", cc.TAGS)
def test_conv_row_vs_float64(tag, nterms):
    from bin_amd import ops
    case = cc.BY_TAG[tag]
    ops.check_status()
    for shape in cc.shapes(case):
        for family in rc.families(nterms):
            opnd = rc.operands(tag, family, shape)
            outs, inputs = cc.call_library(case, nterms, shape, opnd)
            got = _decoded(outs)
            _check_uploaded(tag, nterms, opnd, inputs)
            if family != "C":
                ops.check_status()           # integers and split-exact values stay far inside the fp16 range
            rc.compare(case, nterms, family, shape, got)
    ops.check_status()


@pytest.mark.parametrize("nterms", cc.NTERMS)
def test_gff0_backward_data_scatters_into_groups(nterms):
    """GFF.0's backward-data as binhip_plan.hip issues it: the 72 output chunks leave as 12 groups of 6 (y_cpg, y_group_stride) — here
    with one gap plane between groups, filled with a guard value that must survive; the group planes against float64 (integers bit
    for bit, white noise within the bars of the unscattered case)."""
    from bin_amd import ops
    case = cc.BY_TAG[rc.SCATTER_TAG]
    cpg, ngroups = rc.SCATTER_CPG, rc.SCATTER_GROUPS
    assert cc.chunks(case.cin) == cpg * ngroups
    ops.check_status()
    for shape in cc.shapes(case):
        n, h, w = shape
        for family in ("A", "C"):
            out = ops.CP.empty(ngroups * (cpg + 1), n, h, w, nterms, torch.device("cuda"))
            out.hi.fill_(rc.GUARD_HI)
            if out.lo is not None:
                out.lo.fill_(rc.GUARD_LO)
            opnd = rc.operands(case.tag, family, shape)
            outs, _ = cc.call_library(case, nterms, shape, opnd, out=out, y_cpg=cpg, y_group_stride=(cpg + 1) * n * h * w * 16)
            y = outs["y"]
            data = [g * (cpg + 1) + i for g in range(ngroups) for i in range(cpg)]
            gaps = [g * (cpg + 1) + cpg for g in range(ngroups)]
            assert bool((y.hi[gaps] == rc.GUARD_HI).all()), (shape, family, "a gap plane was written (hi)")
            if y.lo is not None:
                assert bool((y.lo[gaps] == rc.GUARD_LO).all()), (shape, family, "a gap plane was written (lo)")
            got = rc.planes_to_nchw(y.hi[data]) + (rc.planes_to_nchw(y.lo[data]) if y.lo is not None else 0)
            print("[conv-f64] the next line: the same row with its output scattered, y_cpg=%d" % cpg)
            rc.compare(case, nterms, family, shape, {"y": got})
            ops.check_status()
