"""GPU: the baselines of tests/abi_cases.py are real calls.

tests/test_cpu_abi_domain.py pins what every libbinhip.so entry point refuses AROUND a baseline; this module proves that the baselines
themselves are valid and that their "bytes the callee may touch" are true.  Every baseline is replayed with device buffers of exactly
the byte size its row declares, each inside the guard bands of tests/poison.py.  A call must return 0 (a host query: its value), leave
the status word clear and leave every guard band intact.  Only baselines run here: no mutation, and nothing from the refused side of a
limit, ever reaches a GPU.  Numerical correctness is held elsewhere (float64 references per kernel); the buffers are zero-filled."""
import pytest
import torch

import abi_cases as A
import poison

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bid", list(A.BASELINES))
def test_baseline_is_a_real_call(bid):
    b = A.BASELINES[bid]
    bufs = {}

    def alloc(name, nbytes, fill):
        assert nbytes > 0, f"{bid}: {name} declares {nbytes} bytes"
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")      # (under `poisoned`: zero payload between two guard bands)
        if fill:
            t.view(torch.float32).fill_(fill)
        bufs[name] = t
        return t.data_ptr()

    with poison.poisoned(0x00) as rec:
        rv, ctx = A.call(bid, {}, alloc)
        torch.cuda.synchronize()
        assert b.accept(rv, True), f"{b.entry} ({bid}) returned {rv}"
        assert rec.count == len(ctx.sizes) == len(bufs)
        assert all(t.data_ptr() % 256 == 0 and t.numel() == ctx.sizes[n] for n, t in bufs.items())
        if "status" in bufs:
            assert int(bufs["status"].view(torch.int32).item()) == 0, f"{bid}: status word {bufs['status'].view(torch.int32).item():#x}"
    # (leaving `poisoned` compared every guard band with poison.GUARD_BYTE: nothing was written outside the declared sizes)


def test_every_entry_point_is_replayed():
    from bin_amd import _lib
    assert {b.entry for b in A.BASELINES.values()} | set(A.EXEMPT) == set(_lib.exported_symbols("binhip"))
