"""Every answer the sixteen mrhip_create_* constructors can give, against the built library on the GPU: the cases of
tests/create_refusal_cases.py (one per refusal of each entry point: out / h NULL, hLen 0, the dtypes, the wrong tap class alone and
together with a NULL h or out -- the order of the first checks differs between the entry points --, nch, the device ordinal, ratio, rate
or rates, Nphi, polyorder) must give the (status, mrhip_last_error()) of tests/golden/create_refusals.json and leave *out NULL; then
each of the sixteen valid filters is created and destroyed once.  No kernel runs.

The JSON was recorded ONCE, on an MI355X, from the library of the commit BEFORE the constructors moved into csrc/create.hip ("Per-channel
rates for FIRFarrow; rates that change between calls"), built in a separate tree and loaded through MRHIP_LIB_PATH, by running
run_case() of tests/create_refusal_cases.py over cases() and writing {id: [status, message]} (message "" for status 0).  It is never
recorded from the code under test: a row that no longer matches is a change of behaviour.

A rank-deficient fit ("polynomial fit is rank deficient") has no case: the fit's matrix is the Vandermonde matrix of the nodes
1..Nphi, which does not depend on the taps and has full column rank whenever polyorder + 1 <= Nphi -- what the check in front of the
fit demands -- so no tap vector, of 8 taps or any other length, reaches that answer through a constructor."""
import ctypes as C
import json
import os

import pytest

import create_refusal_cases as cr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_refusals.json")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def test_every_case_answers_as_recorded(pkg, torch_cuda):
    lib = pkg.load_library()
    want = json.load(open(GOLDEN))
    cases = cr.cases()
    assert sorted(want) == sorted(c[0] for c in cases)                       # the table and the case list name the same cases
    buffers = cr.Buffers()
    differing, not_cleared = [], []
    for case_id, name, stage, changes in cases:
        status, message, cleared = cr.run_case(lib, name, changes, buffers, torch_cuda.cuda.device_count())
        if [status, message] != want[case_id]:
            differing.append((case_id, [status, message], want[case_id]))
        if status != 0 and not cleared:
            not_cleared.append(case_id)
    assert not differing, differing[:8]
    assert not not_cleared, not_cleared[:8]


@pytest.mark.parametrize("name", list(cr.ENTRIES))
def test_the_valid_call_makes_a_filter(pkg, torch_cuda, name):
    lib = pkg.load_library()
    buffers = cr.Buffers()
    args, out, keep = cr.call_args(name, {}, buffers)
    assert getattr(lib, name)(*args) == 0, lib.mrhip_last_error()
    assert out.value and out.value != 0xdead0
    family, taps, bank, rates, pnfb, _ = cr.ENTRIES[name]
    if rates:                                                                # a state per channel (one state: status 5 on such a filter)
        states = (pkg.host.ChannelState * cr.NCH)()
        assert lib.mrhip_get_channel_states(out, states) == 0, lib.mrhip_last_error()
        assert [(s.rate, s.delta, s.phiAccumulator, s.inputDeficit) for s in states] == [(r, cr.NPHI / r, 1.0, 1) for r in cr.RATES]
    else:
        st = pkg.host._State()
        assert lib.mrhip_get_state(out, C.byref(st)) == 0, lib.mrhip_last_error()
        assert st.nchannels == cr.NCH and st.hLen == cr.HLEN and st.tap_dtype == args[2]
        assert (st.kind == 3) if family == "rational" else (st.kind == {"arbitrary": 4, "farrow": 5}[family] and st.Nphi == cr.NPHI and st.tapsPerPhi == 2)
    lib.mrhip_destroy(out)
