"""CPU-only checks of the per-channel-taps feature (FIRFilter.per_channel, mrhip_create_rational_bank, csrc/kernels_bank.hip): the
argument errors of the Python constructor, the build conditions of the kernel unit (as tests/test_build_properties_ctaps_farrow.py
checks them) and the instantiations in the object the build made: both kernels for (Tx scalar, R) in {(f32,f32), (f32,f64), (f64,f64)}
x real / complex samples x STRICT / FUSED = 12 each, none with scratch memory or AccVGPRs."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch


def test_argument_errors_of_the_python_constructor(pkg):
    H = np.ones((3, 8), dtype=np.float32)
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(H[0], Fraction(3, 5))             # not 2-D
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(np.ones((2, 3, 4), dtype=np.float32), Fraction(3, 5))
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(H, 1.5)                           # a float rate: the rational family only
    assert e.value.code == 5
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel(H.astype(ct), Fraction(3, 5))  # complex taps in a bank
        assert e.value.code == 5


def test_the_unbound_filter_describes_one_channels_filter(pkg):
    H = np.arange(3 * 11, dtype=np.float64).reshape(3, 11)
    f = pkg.FIRFilter.per_channel(H, Fraction(6, 10))
    st = f.state
    assert (f.kind, st.interpolation, st.decimation, st.hLen, st.tapsPerPhi, st.historyLen) == (pkg.FIRFilter(H[0], Fraction(3, 5)).kind, 3, 5, 11, 4, 3)
    assert pkg.FIRFilter.per_channel(H, 1).kernel_name == pkg.FIRFilter(H[0], 1).kernel_name


def test_the_library_exports_the_constructor(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "mrhip_create_rational_bank")
    hdr = open(os.path.join(os.path.dirname(CSRC), "..", "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_create_rational_bank\(const void \*h, int64_t hLen, int tap_dtype, int64_t num, int64_t den,\s*"
                     r"int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_bank\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    src = open(os.path.join(CSRC, "kernels_bank.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    # FUSED is an explicit fma: the unit's multiply-add is RealTaps::step of variant_device.h, which calls mac of pipe_stage.h
    shared = open(os.path.join(CSRC, "variant_device.h")).read()
    assert '#include "variant_device.h"' in src and "RealTaps<TX, R, NCX, FUSED>" in src
    assert '#include "pipe_stage.h"' in shared and "#pragma clang fp contract(off)" in shared and "mac<FUSED, R>(" in shared
    mac = open(os.path.join(CSRC, "pipe_stage.h")).read()
    assert "__builtin_fmaf" in mac and "__builtin_fma(" in mac


def test_bank_kernels_use_no_scratch(pkg):
    src = "kernels_bank.hip"
    obj = os.path.join(CSRC, "build", src + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    if os.path.getmtime(obj) < os.path.getmtime(os.path.join(CSRC, src)):
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel, count in (("poly_bank_generic_kernel", 12), ("poly_bank_tiled_kernel", 12)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"
