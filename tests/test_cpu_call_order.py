"""The scenario table and the float64 reference of tests/test_gpu_call_order.py, checked without a GPU: the table is well formed, the
clean-run builder replays `update` steps deterministically, and the float64 gradient is additive over micro-batches (the accumulation test
compares the device's sum of two backward calls with the float64 gradient of the summed loss)."""
import torch

import call_order_cases as CO
from backward_cases import RDN_CASES, rel


def test_scenario_table_is_well_formed():
    cases = CO.cases()
    assert len({cid for cid, *_ in cases}) == len(cases) > 30
    sizes = {tuple(v[2:4]) for v in RDN_CASES.values()}
    assert all(s[1:] in sizes for s in CO.SHAPES)                                # frame sizes of the ragged-shape table
    for cid, k, mode, sc in cases:
        assert CO.check_scenario(sc), cid
        assert k in (2, 3, 5) and mode in ("f16x3", "mixed", "two_layer")
        kind, shape, updates, prec = CO.probe_context(sc)
        clean = {"steps": CO.clean_steps(sc), "probe": sc["probe"], "also": ()}
        assert CO.check_scenario(clean), cid
        assert CO.probe_context(clean) == (kind, shape, updates, prec), cid      # the clean run reproduces the probe's context
        assert [s for s in clean["steps"] if s[0] in ("eval", "train_fwd")][0][1] == sc["probe"]
    names = {cid.split("-")[0] for cid, *_ in cases}
    for n in "1234567":
        assert any(x.startswith(n + "_") for x in names), f"scenario {n} missing"
    for starred in ("1_eval_then_train", "2_validation_after_update"):
        assert {k for cid, k, _, _ in cases if cid.startswith(starred)} == {2, 3, 5}
    assert {m for cid, _, m, _ in cases if cid.startswith("4_")} == {"f16x3", "mixed"}
    # malformed tables are refused
    for bad in ([("bwd", "p")], [("train_fwd", "p", CO.SMALL), ("bwd", "p"), ("bwd", "p")], [("train_fwd", "p", CO.SMALL), ("drop", "p")],
                [("train_fwd", "p", CO.SMALL)]):
        try:
            CO.check_scenario({"steps": bad, "probe": "p", "also": ()})
        except AssertionError:
            continue
        raise AssertionError(f"accepted {bad}")


def test_updates_replay_deterministically(canon_cpu):
    """The same seed gives the same perturbation (compared as tensors), different seeds and different parameters different ones, and the
    module-side `apply_update` lands on exactly the weights `updated_weights` states for the float64 reference."""
    w = CO.local_weights(canon_cpu, 2)
    a, b, c = CO.perturbation(w, 1), CO.perturbation(w, 1), CO.perturbation(w, 2)
    assert set(a) == set(w) and len(a) == 132
    assert all(torch.equal(a[n], b[n]) for n in a)
    assert all(not torch.equal(a[n], c[n]) for n in a)
    assert not torch.equal(a["RDBs.0.LFF.bias"], a["RDBs.1.LFF.bias"])
    assert all(a[n].dtype == torch.float32 and 0 < float(a[n].abs().max()) <= 6 * CO.UPDATE_SCALE * float(w[n].abs().max()) for n in a)
    u1, u2 = CO.updated_weights(canon_cpu, 2, (1, 2)), CO.updated_weights(canon_cpu, 2, (1, 2))
    assert all(torch.equal(u1[n], u2[n]) for n in u1)
    assert all(torch.equal(w[n], canon_cpu[f"model1.{n}"]) for n in w), "updated_weights changed the canonical set"

    class Holder(torch.nn.Module):            # apply_update needs named_parameters() only
        def __init__(self):
            super().__init__()
            self.p = torch.nn.ParameterDict({n.replace(".", "_"): torch.nn.Parameter(t.clone()) for n, t in list(w.items())[:6]})
    h = Holder()
    versions = [p._version for p in h.parameters()]
    CO.apply_update(h, 1)
    CO.apply_update(h, 2)
    assert all(p._version > v for p, v in zip(h.parameters(), versions))
    ref = {n: t.clone() for n, t in h.named_parameters()}
    h2 = Holder()
    CO.apply_update(h2, 1)
    CO.apply_update(h2, 2)
    assert all(torch.equal(p, ref[n]) for n, p in h2.named_parameters())


def test_float64_reference_is_additive_over_micro_batches(canon_cpu):
    """At (1, 12, 14): the float64 gradient of the summed loss of two micro-batches (one call on the concatenated batch) equals the sum of
    the two calls' gradients to 1e-12 relative; the frame gradients are the two calls' own."""
    k, shape = 2, (1, 12, 14)
    w = CO.local_weights(canon_cpu, k)
    (ia, ga), (ib, gb) = CO.inputs(k, shape, 0), CO.inputs(k, shape, 1)
    ma, mb = CO.float64_masks(w, k, ia), CO.float64_masks(w, k, ib)
    assert len(ma) == 48
    ra = CO.oracle_grads(w, k, ia, ga, ma, "a")
    rb = CO.oracle_grads(w, k, ib, gb, mb, "b")
    both = CO.oracle_grads(w, k, [torch.cat((x, y)) for x, y in zip(ia, ib)], torch.cat((ga, gb)),
                           [torch.cat((x, y)) for x, y in zip(ma, mb)], "a + b")
    worst = 0.0
    for n in w:
        worst = max(worst, rel(ra[n] + rb[n], both[n]))
    for j in range(k):
        worst = max(worst, rel(torch.cat((ra[f"in{j}"], rb[f"in{j}"])), both[f"in{j}"]))
    print(f"float64 additivity over two micro-batches: worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    assert min(float(ra[n].abs().max()) for n in w) > 0
