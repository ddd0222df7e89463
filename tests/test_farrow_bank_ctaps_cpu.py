"""CPU-only checks of per-channel complex taps for FIRFarrow (FIRFilter.per_channel_complex_taps_farrow,
mrhip_create_farrow_bank_ctaps, csrc/kernels_bank_farrow_ctaps.hip): the argument errors of the Python constructor, the refusals the
older constructors keep, the description of the unbound filter, the exported symbol and its declaration, the build conditions of the
kernel unit and the instantiations in the object the build made: the one new kernel for (Tx scalar, R) in {(f32,f32), (f32,f64),
(f64,f64)} x real / complex samples = 6, none with scratch memory or AccVGPRs.  (kernels_bank_farrow.hip, the unit it was modelled on,
is unchanged -- the shared body of variant_device.h serves the new kernel only -- and tests/test_farrow_bank_cpu.py keeps counting its
12 + 12.)"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch


def test_argument_errors_of_the_python_constructor(pkg):
    H = np.ones((3, 8), dtype=np.complex64)
    for bad in (H[0], np.ones((2, 3, 4), dtype=np.complex64), np.ones((0, 4), dtype=np.complex64), np.ones((2, 0), dtype=np.complex64)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_farrow(bad, 1.5, 4, 2)      # not a (nchannels >= 1, hLen >= 1) matrix
        assert e.value.code == 1
    for rt in (np.float32, np.float64):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_farrow(H.real.astype(rt), 1.5, 4, 2)   # real taps: per_channel_farrow
        assert e.value.code == 1 and "per_channel_farrow" in str(e.value)
    for rate in (Fraction(3, 2), 2, (3, 2)):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_farrow(H, rate, 4, 2)       # a ratio: per_channel_complex_taps
        assert e.value.code == 1 and "per_channel_complex_taps" in str(e.value)
    for rate in (-1.5, 0.0):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_complex_taps_farrow(H, rate, 4, 2)       # "rate must be greater than 0", Filters.jl:193
        assert e.value.code == 1
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps_farrow(H, 1.5, 4, None)         # no polyorder: that is FIRArbitrary
    assert e.value.code == 1 and "per_channel_complex_taps_arbitrary" in str(e.value)
    with pytest.raises(TypeError):
        pkg.FIRFilter.per_channel_complex_taps_farrow(H, 1.5, 4, 2, numerics=pkg.NUMERICS_FUSED)   # there is no numerics argument
    with pytest.raises(TypeError):
        pkg.FIRFilter.per_channel_complex_taps_farrow(H, 1.5, 4, 2, pnfb=np.zeros((2, 3), dtype=np.complex128))   # nor a caller-fitted bank


def test_the_older_constructors_keep_their_refusals_and_name_the_new_one(pkg):
    H = np.ones((3, 8), dtype=np.complex64)
    for ct in (np.complex64, np.complex128):
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_farrow(H.astype(ct), 1.5, 4, 2)          # complex taps: not through this constructor
        assert e.value.code == 5 and "per_channel_complex_taps_farrow" in str(e.value)
        with pytest.raises(pkg.MultirateHIPError) as e:
            pkg.FIRFilter.per_channel_arbitrary(H.astype(ct), 1.5)
        assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps(H, 1.5)                         # a float rate: not the rational family
    assert e.value.code == 5 and "per_channel_complex_taps_farrow" in str(e.value) and "per_channel_complex_taps_arbitrary" in str(e.value)
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(H.real.astype(np.float32), 1.5)              # a float rate: not the rational family
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel(H, 2)                                        # complex taps: per_channel_complex_taps
    assert e.value.code == 5
    with pytest.raises(pkg.MultirateHIPError) as e:
        pkg.FIRFilter.per_channel_complex_taps_arbitrary(H, Fraction(3, 2))
    assert e.value.code == 1


def test_the_unbound_filter_describes_one_channels_filter(pkg):
    H = (np.arange(3 * 30).reshape(3, 30) * (1 - 2j)).astype(np.complex128)
    f = pkg.FIRFilter.per_channel_complex_taps_farrow(H, 2.123, 4, 3)
    one = pkg.FIRFilter.complex_taps_farrow(H[0], 2.123, 4, 3)
    st = f.state
    assert f.kind == one.kind == pkg.host.FARROW and f.kernel_name == one.kernel_name
    assert (st.kind, st.Nphi, st.hLen, st.tapsPerPhi, st.historyLen) == (5, 4, 30, 8, 7)             # tapsPerPhi = ceil(hLen / Nphi)
    assert (st.rate, st.delta, st.phiAccumulator, st.inputDeficit) == (2.123, 4 / 2.123, 1.0, 1)     # delta = Nphi / rate; the constructor state
    assert f.polyorder == one.polyorder == 3
    assert f.numerics == pkg.NUMERICS_STRICT
    d = pkg.FIRFilter.per_channel_complex_taps_farrow(H.astype(np.complex64), 0.47)
    assert (d.Nphi, d.polyorder) == (32, 4)                                                          # the defaults
    assert d._bank.dtype == np.complex64
    assert np.array_equal(f._bank, H) and f._bank is not H and f._bank.dtype == np.complex128        # copied, in the tap type
    assert np.array_equal(f.h, H[0])


def test_the_library_exports_the_constructor_and_the_header_declares_it(pkg):
    lib = pkg.load_library()
    assert hasattr(lib, "mrhip_create_farrow_bank_ctaps")
    rows = [(res, args) for name, res, args in pkg.host.ABI if name == "mrhip_create_farrow_bank_ctaps"]
    same = [(res, args) for name, res, args in pkg.host.ABI if name == "mrhip_create_farrow_bank"]
    assert len(rows) == 1 and rows == same                                  # the signature of its real-tap neighbour
    assert lib.mrhip_abi_version() == 1
    hdr = open(os.path.join(os.path.dirname(CSRC), "..", "include", "multirate_hip.h")).read()
    assert re.search(r"int mrhip_create_farrow_bank_ctaps\(const void \*h, int64_t hLen, int tap_dtype, double rate, int64_t Nphi,\s*"
                     r"int64_t polyorder,\s*int sample_dtype, int64_t nchannels, int device, mrhip_filter \*\*out\);", hdr)
    assert "Per-channel complex taps for FIRFarrow" in hdr
    for accessor in ("mrhip_get_pnfb", "mrhip_farrow_tapsforphase"):         # their comments name the new constructor
        comment = hdr[:hdr.index("int " + accessor + "(")].rsplit("/*", 1)[1]
        assert "mrhip_create_farrow_bank_ctaps" in comment, accessor


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_bank_farrow_ctaps\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"^.*kernels_bank_farrow_ctaps\.hip\.o.*:\s*ctaps_device\.h\s*$", mk, flags=re.M)   # rebuilt when the shared arithmetic changes
    src = open(os.path.join(CSRC, "kernels_bank_farrow_ctaps.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert '#include "variant_device.h"' in src
    assert "farrow_variant_bank_generic_body<ComplexTaps<TX, R, NCX>>" in src
    assert "launch_lane_per_output(" in src
    assert "asm" not in src                                                  # plain HIP
    shared = open(os.path.join(CSRC, "variant_device.h")).read()
    assert "#pragma clang fp contract(off)" in shared and "farrow_variant_bank_generic_body" in shared
    assert "address_space(4)" in shared and "kFarrowBankUnrolledP = 4" in shared   # the coefficients through the constant address space


def _scratch_of(src):
    obj = os.path.join(CSRC, "build", src + ".o")
    assert os.path.exists(obj), "no built object: " + obj
    assert os.path.exists(os.path.join(LLVM, "llvm-readelf")), "no llvm tools"
    newest = max(os.path.getmtime(os.path.join(CSRC, s)) for s in (src, "variant_device.h", "ctaps_device.h"))
    assert os.path.getmtime(obj) >= newest, "object older than its source: build again"
    return _kernel_scratch(obj)


def test_the_one_kernel_has_six_instantiations_without_scratch(pkg):
    sizes = _scratch_of("kernels_bank_farrow_ctaps.hip")
    mine = {k: v for k, v in sizes.items() if "farrow_bank_ctaps_generic_kernel" in k}
    assert len(mine) == 6, f"expected 6 instantiations of farrow_bank_ctaps_generic_kernel in the object, found {len(mine)}"
    assert len(sizes) == 6, f"kernels other than the one: {sorted(set(sizes) - set(mine))}"        # no second kernel
    spilling = {k: v for k, v in mine.items() if v != 0}
    assert not spilling, f"instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"

