"""CPU-only checks of the per-channel complex-taps feature (FIRFilter.per_channel_complex_taps, mrhip_create_rational_bank_ctaps,
csrc/kernels_bank_ctaps.hip): the argument errors of the Python constructor, the build conditions of the kernel unit (as
tests/test_bank_cpu.py checks them for the real-tap unit) and the instantiations in the object the build made: both kernels for (Tx scalar, R)
in {(f32,f32), (f32,f64), (f64,f64)} x real / complex samples = 6 each, none with scratch memory or AccVGPRs."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch


def test_argument_errors_of_the_python_constructor(pkg):
    H = np.ones((3, 8), dtype=np.complex64)
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps(H[0], Fraction(3, 5))             # not 2-D
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps(np.ones((2, 3, 4), dtype=np.complex64), Fraction(3, 5))
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps(np.ones((0, 4), dtype=np.complex64), Fraction(3, 5))
    assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps(H, 1.5)                           # a float rate: the rational family only
    assert e.value.code == 5
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel(H.astype(ct), Fraction(3, 5))              # the real-tap constructor keeps refusing
        assert e.value.code == 5


def test_real_taps_are_promoted_to_complex_as_complex_taps_does(pkg):
    for rt, ct in ((np.float32, np.complex64), (np.float64, np.complex128), (np.int32, np.complex128)):
        f = pkg.FIRFilter.per_channel_complex_taps(np.arange(6).reshape(2, 3).astype(rt), Fraction(1, 2))
        assert f.h.dtype == ct and f._bank.dtype == ct and f._bank.shape == (2, 3)
        assert f.h.dtype == pkg.FIRFilter.complex_taps(np.arange(3).astype(rt), Fraction(1, 2)).h.dtype
        assert f.numerics == pkg.NUMERICS_STRICT


def test_the_unbound_filter_describes_one_channels_filter(pkg):
    H = (np.arange(3 * 11, dtype=np.float64).reshape(3, 11) * (1 - 2j)).astype(np.complex128)
    f = pkg.FIRFilter.per_channel_complex_taps(H, Fraction(6, 10))
    st = f.state
    assert (f.kind, st.interpolation, st.decimation, st.hLen, st.tapsPerPhi, st.historyLen) == \
        (pkg.FIRFilter.complex_taps(H[0], Fraction(3, 5)).kind, 3, 5, 11, 4, 3)
    assert pkg.FIRFilter.per_channel_complex_taps(H, 1).kernel_name == pkg.FIRFilter.complex_taps(H[0], 1).kernel_name
    assert pkg.FIRFilter.per_channel_complex_taps(H, Fraction(1, 4)).kernel_name == pkg.FIRFilter.complex_taps(H[0], Fraction(1, 4)).kernel_name


def test_the_library_exports_the_constructor(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "mrhip_create_rational_bank_ctaps")
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(os.path.dirname(CSRC), "..", "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_create_rational_bank_ctaps\(const void \*h, int64_t hLen, int tap_dtype, int64_t num, int64_t den,\s*"
                     r"int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)
    assert "Per-channel complex taps" in hdr


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_bank_ctaps\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_bank_ctaps\.hip\.o.*:\s*ctaps_device\.h\s*$", mk, flags=re.M)   # rebuilt when the shared arithmetic changes
    src = open(os.path.join(CSRC, "kernels_bank_ctaps.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "ctaps_device.h"' in src
    assert "fma" not in src                                          # no FUSED form; the arithmetic is ctaps_device.h's alone


def test_bank_ctaps_kernels_use_no_scratch(pkg):
    src = "kernels_bank_ctaps.hip"
    obj = os.path.join(CSRC, "build", src + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    if os.path.getmtime(obj) < os.path.getmtime(os.path.join(CSRC, src)):
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel, count in (("poly_bank_ctaps_generic_kernel", 6), ("poly_bank_ctaps_tiled_kernel", 6)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"
