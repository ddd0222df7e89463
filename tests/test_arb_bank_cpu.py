"""CPU-only checks of per-channel taps for FIRArbitrary (FIRFilter.per_channel_arbitrary, mrhip_create_arbitrary_bank,
csrc/kernels_bank_arb.hip): the argument errors of the Python constructor, the description of the unbound filter, the exported symbol
and its declaration, the build conditions of the kernel unit and the instantiations in the object the build made: both kernels for
(Tx scalar, R) in {(f32,f32), (f32,f64), (f64,f64)} x real / complex samples x STRICT / FUSED = 12 each, none with scratch memory or
AccVGPRs."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch


def test_argument_errors_of_the_python_constructor(pkg):
    H = np.ones((3, 8), dtype=np.float32)
    for bad in (H[0], np.ones((2, 3, 4), dtype=np.float32), np.ones((0, 4), dtype=np.float32), np.ones((2, 0), dtype=np.float32)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_arbitrary(bad, 1.5)              # not a (nchannels >= 1, hLen >= 1) matrix
        assert e.value.code == 1
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_arbitrary(H.astype(ct), 1.5)     # complex taps in a FIRArbitrary bank: left out
        assert e.value.code == 5
    for rate in (Fraction(3, 2), 2, (3, 2)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_arbitrary(H, rate)               # a ratio: FIRFilter.per_channel
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_arbitrary(H, -1.5)                   # "rate must be greater than 0", Filters.jl:184
    assert e.value.code == 1


def test_per_channel_with_a_float_rate_keeps_raising_unsupported(pkg):
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(np.ones((3, 8), dtype=np.float32), 1.5)
    assert e.value.code == 5


def test_the_unbound_filter_describes_one_channels_filter(pkg):
    H = np.arange(3 * 30, dtype=np.float64).reshape(3, 30)
    f = pkg.FIRFilter.per_channel_arbitrary(H, 2.123, 4, numerics=pkg.NUMERICS_FUSED)
    one = pkg.FIRFilter(H[0], 2.123, 4)
    st = f.state
    assert f.kind == one.kind == pkg.host.ARBITRARY and f.kernel_name == one.kernel_name
    assert (st.kind, st.Nphi, st.hLen, st.tapsPerPhi, st.historyLen) == (4, 4, 30, 8, 7)             # tapsPerPhi = ceil(hLen / Nphi)
    assert (st.rate, st.delta, st.phiAccumulator, st.inputDeficit) == (2.123, 4 / 2.123, 1.0, 1)
    assert f.numerics == pkg.NUMERICS_FUSED
    assert pkg.FIRFilter.per_channel_arbitrary(H.astype(np.float32), 0.47).Nphi == 32               # Nphi defaults to 32
    assert np.array_equal(f._bank, H) and f._bank is not H


def test_the_library_exports_the_constructor_and_the_header_declares_it(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "mrhip_create_arbitrary_bank")
    assert any(name == "mrhip_create_arbitrary_bank" for name, *_ in pkg.host.ABI)
    hdr = open(os.path.join(os.path.dirname(CSRC), "..", "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_create_arbitrary_bank\(const void \*h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,\s*"
                     r"int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_bank_arb\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    src = open(os.path.join(CSRC, "kernels_bank_arb.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    # FUSED is an explicit fma: the unit's multiply-add is RealTaps::step of variant_device.h, which calls mac of pipe_stage.h
    shared = open(os.path.join(CSRC, "variant_device.h")).read()
    assert '#include "variant_device.h"' in src and "RealTaps<TX, R, NCX, FUSED>" in src
    assert '#include "pipe_stage.h"' in shared and "#pragma clang fp contract(off)" in shared and "mac<FUSED, R>(" in shared
    mac = open(os.path.join(CSRC, "pipe_stage.h")).read()
    assert "__builtin_fmaf" in mac and "__builtin_fma(" in mac


def test_arb_bank_kernels_use_no_scratch(pkg):
    src = "kernels_bank_arb.hip"
    obj = os.path.join(CSRC, "build", src + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    if os.path.getmtime(obj) < os.path.getmtime(os.path.join(CSRC, src)):
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel, count in (("arb_bank_generic_kernel", 12), ("arb_bank_tiled_kernel", 12)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"
