"""CPU: what every libbinhip.so entry point refuses before it launches (tests/abi_cases.py, one row per entry point).

THIS MODULE RUNS ONLY WHERE NOTHING CAN LAUNCH.  It makes ACCEPTED calls that carry dummy addresses: on a machine with a GPU they
would be kernels reading and writing those addresses.  The whole module is therefore skipped unless BOTH hold: torch sees no GPU
(`torch.cuda.is_available()` is false) and the library itself finds none (`binhip_device_cus() <= 0`).  It is not marked `gpu`: it is
the CPU half; tests/test_gpu_abi_baselines.py replays the baselines (and nothing else) with real buffers on a GPU.

Without a device an accepted call passes validation and returns the positive hipError_t of its first HIP call; a refused call returns
exactly its BINHIP_E_* code."""
import pytest
import torch

import abi_cases as A
from bin_amd import _lib as L


def _nothing_can_launch():
    if torch.cuda.is_available():
        return False
    try:
        return L.lib().binhip_device_cus() <= 0
    except (RuntimeError, OSError):           # not built yet at collection time: the session fixture builds it; decide again there
        return None


_SAFE = _nothing_can_launch()
pytestmark = pytest.mark.skipif(_SAFE is False, reason="accepted calls with dummy addresses must never run where a launch could succeed")


@pytest.fixture(autouse=True)
def _no_device():
    if torch.cuda.is_available() or L.lib().binhip_device_cus() > 0:
        pytest.skip("a device is present: accepted calls with dummy addresses must not run")


def _what(over):
    return ",".join(f"{k}={v.__name__ if callable(v) else v}" for k, v in over.items()) or "baseline"


def _run(base, over):
    rv, ctx = A.call(base, over, A.dummy_alloc())
    return rv


def test_every_exported_symbol_has_a_row():
    """One row per entry point; the four that take nothing that can be wrong are exempt, and that list is held here literally."""
    exempt = ("binhip_version", "binhip_device_cus", "binhip_charbonnier_partials", "binhip_profiler_destroy")
    assert tuple(A.EXEMPT) == exempt
    rows = {b.entry for b in A.BASELINES.values()}
    assert rows | set(exempt) == set(L.exported_symbols("binhip")), rows ^ (set(L.exported_symbols("binhip")) - set(exempt))
    assert not rows & set(exempt)
    refused = {A.BASELINES[m.base].entry for m in A.MUTATIONS} | {A.BASELINES[m.base].entry for m in A.LIMITS if m.bad is not None}
    assert refused == rows, f"entry points without a single refusal in the table: {sorted(rows - refused)}"
    assert len({(m.base, _what(m.over)) for m in A.MUTATIONS}) == len(A.MUTATIONS), "a mutation is listed twice"


def test_baselines_use_distinct_aligned_dummy_addresses():
    for bid in A.BASELINES:
        if not A.BASELINES[bid].cpu:
            continue
        seen = []
        alloc = A.dummy_alloc()
        _, _, ctx = A.materialise(bid, {}, lambda n, b, f: seen.append(alloc(n, b, f)) or seen[-1])
        assert all(a and a % 256 == 0 for a in seen) and len(set(seen)) == len(seen), bid
        assert all(n >= 0 for n in ctx.sizes.values()), (bid, ctx.sizes)


@pytest.mark.parametrize("bid", [b for b in A.BASELINES if A.BASELINES[b].cpu])
def test_baseline_is_accepted(bid):
    """Validation passes and the launch finds no device: a code > 0 (a pure host query: its value)."""
    rv = _run(bid, {})
    assert A.BASELINES[bid].accept(rv, False), f"{bid}: returned {rv}"
    if A.BASELINES[bid].accept is A.launched:
        assert rv > 0


@pytest.mark.parametrize("i", range(len(A.MUTATIONS)), ids=[f"{m.base}:{_what(m.over)}" for m in A.MUTATIONS])
def test_mutation_is_refused(i):
    m = A.MUTATIONS[i]
    rv = _run(m.base, m.over)
    assert rv == m.code, f"{A.BASELINES[m.base].entry} with {_what(m.over)} returned {rv}, expected {m.code}: {m.why}"


@pytest.mark.parametrize("i", range(len(A.LIMITS)), ids=[f"{m.base}:{_what(m.ok)}|{_what(m.bad or {})}" for m in A.LIMITS])
def test_both_sides_of_a_limit(i):
    """The last legal value is accepted, the first illegal one refused (`bad` None: a value the header defines, accepted)."""
    m = A.LIMITS[i]
    b = A.BASELINES[m.base]
    rv = _run(m.base, m.ok)
    assert b.accept(rv, False), f"{b.entry} with {_what(m.ok)} returned {rv}, expected acceptance: {m.why}"
    if m.bad is not None:
        rv = _run(m.base, m.bad)
        assert rv == m.code, f"{b.entry} with {_what(m.bad)} returned {rv}, expected {m.code}: {m.why}"


@pytest.mark.parametrize("i", range(len(A.WORKSPACES)), ids=[w.base for w in A.WORKSPACES])
def test_workspace_query_and_call_agree(i):
    w = A.WORKSPACES[i]
    query = getattr(L.lib(), w.query)

    def size(over):
        c = A.Ctx(over, A.dummy_alloc())
        return query(*w.qargs(c))
    need = size({})
    assert need > 0
    for geo in w.refused:
        assert size(geo) == 0, f"{w.query} is non-zero for {geo}"
        assert _run(w.base, geo) < 0, f"{w.base} accepts {geo}"
    assert _run(w.base, {w.size_name: need - 1}) == A.E_WS
    assert _run(w.base, {w.size_name: 0}) == A.E_WS
    assert _run(w.base, {w.size_name: need}) > 0


def test_table_names_its_limits_through_the_binding():
    """A limit the header changes moves the rows with it: the table's constants are the binding's mirrors of the #defines."""
    import os
    import re
    from conftest import REPO
    hdr = open(os.path.join(REPO, "include", "binhip.h")).read()

    def define(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert L.LOSS_MAX_TERMS == define("BINHIP_LOSS_MAX_TERMS") and L.SCORE_MAX_PAIRS == define("BINHIP_SCORE_MAX_PAIRS")
    assert L.RDN_MAX_CONVS == define("BINHIP_RDN_MAX_CONVS") and L.RDN_MAX_LAYERS == define("BINHIP_RDN_MAX_LAYERS")
    assert L.RDN_LAYOUT_WORDS == define("BINHIP_RDN_LAYOUT_WORDS") and L.RDN_BWD_LAYOUT_WORDS == define("BINHIP_RDN_BWD_LAYOUT_WORDS")
    used = {k for m in A.LIMITS for k in list(m.ok) + list(m.bad or {})}
    for name in ("n_images", "y_cpg", "n_terms", "n_out", "n_slots", "max_launches", "g.term_a[2]", "g.term_b[1]", "cin", "ch", "cw", "top"):
        assert name in used, f"no limit pair for {name}"
