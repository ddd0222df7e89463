"""Build conditions of csrc/kernels_ctaps_farrow.hip (CPU only: reads the object the build made, as tests/test_build_properties.py
does for the pipe kernels): every instantiation of both kernels is in the object -- 6 type combinations of the universal kernel,
6 x CPL in {1, 2} of the tiled one -- none uses scratch memory or AccVGPRs, and the unit is built with -ffp-contract=off (every
multiply and add of the contract is rounded separately)."""
import os
import re

import pytest

from test_build_properties import CSRC, LLVM, _kernel_scratch


def test_complex_tap_farrow_kernels_use_no_scratch(pkg):
    src = "kernels_ctaps_farrow.hip"
    obj = os.path.join(CSRC, "build", src + ".o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no built object (the library came prebuilt) or no llvm tools")
    if os.path.getmtime(obj) < os.path.getmtime(os.path.join(CSRC, src)):
        pytest.skip("object older than its source")
    sizes = _kernel_scratch(obj)
    for kernel, count in (("farrow_ctaps_generic_kernel", 6), ("farrow_ctaps_tiled_kernel", 12)):
        mine = {k: v for k, v in sizes.items() if kernel in k}
        assert len(mine) == count, f"expected {count} instantiations of {kernel} in the object, found {len(mine)}"
        spilling = {k: v for k, v in mine.items() if v != 0}
        assert not spilling, f"{kernel}: instantiations with scratch or AccVGPRs: {list(spilling.items())[:6]}"


def test_the_unit_is_in_the_makefile_with_separately_rounded_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bkernels_ctaps_farrow\.hip\b", mk, flags=re.M)
    assert re.search(r"^CXXFLAGS\s*=.*-ffp-contract=off", mk, flags=re.M)
    assert re.search(r"kernels_ctaps_farrow\.hip\.o[^\n]*: ctaps_device\.h", mk)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "kernels_ctaps_farrow.hip")).read()
