"""CPU tests of tests/output_bounds_cases.py: the case table names exactly the kernels the sources name, its call lengths have the
counts the GPU test relies on, and the checker of the poisoned buffer sees every kind of stray write (and accepts a clean buffer)."""
import numpy as np
import pytest

import output_bounds_cases as B


def test_the_table_names_exactly_the_kernels_of_the_sources():
    """a kernel added to csrc without a bounds case fails here; so does a name in the table that no source has"""
    in_src = B.kernel_names_in_csrc()
    assert len(in_src) >= 32, sorted(in_src)
    assert set(B.CASES) == in_src, (sorted(in_src - set(B.CASES)), sorted(set(B.CASES) - in_src))


def test_store_paths_that_need_a_case_of_their_own_have_one():
    ids = {c.id: c for c in B.ALL_CASES}
    opair = B.CASES["rational_opair_kernel"]
    assert {(np.dtype(c.tx).name) for c in opair} >= {"float32", "complex64", "float64", "complex128"}
    assert any(c.L > 512 for c in opair)
    stream = B.CASES["fir_stream_kernel"]
    f32 = [c for c in stream if c.tx is B.F32]
    assert any(c.M % 2 == 1 for c in f32) and any(c.M % 4 == 2 for c in f32) and any(c.M % 4 == 0 for c in f32)   # odd, even (linear), padded
    assert any(c.tx is B.C64 and c.M == 4 and c.hlen == 128 for c in stream)
    rt = {dict(c.env).get("MRHIP_STREAM_RT_SINGLE") for c in B.CASES["fir_stream_rt_kernel"]}
    assert {"0", "1"} <= rt
    for k in ("arb_pipe_kernel", "farrow_pipe_kernel"):
        assert any(c.tx is B.C64 for c in B.CASES[k]) and any(np.dtype(c.tx).kind == "f" for c in B.CASES[k])
    for k in ("arb_lane_kernel", "interp_lane_kernel"):
        assert {c.nch for c in B.CASES[k]} == {64, 50}
    for c in ids.values():
        assert c.nch <= B.MAX_CHANNELS_OUTSIDE_LANE or c.kernel in ("arb_lane_kernel", "interp_lane_kernel"), c.id
        assert c.min_count >= 768


@pytest.mark.parametrize("case", B.ALL_CASES, ids=lambda c: c.id)
def test_call_lengths_have_an_odd_and_an_even_count_a_short_call_and_an_empty_one(O, case):
    sizes = B.plan_sizes(O, case)
    counts = B.call_counts(O, case, sizes)
    na, n_none, n_few, nb = sizes
    assert sum(sizes) <= B.MAX_SIGNAL, (sizes, counts)
    interp_even = case.kind == "rational" and case.M == 1 and case.L % 2 == 0
    assert (na % 2 == 1 and nb % 2 == 0) if interp_even else (counts[0] % 2 == 1 and counts[3] % 2 == 0), (sizes, counts)
    assert counts[0] % 64 and counts[3] % 64 and counts[0] > 2 * 384 and counts[3] > 2 * 384, (sizes, counts)
    assert counts[1] == 0 and counts[2] >= 1, (sizes, counts)
    if not (case.kind == "rational" and case.L > 1) and not (case.kind != "rational" and case.ratio > 1.0):
        assert counts[2] == 1, (sizes, counts)          # one output wherever a sample does not give several
    p = B.odd_piece(O, case, sum(sizes), sum(sizes) // 3)
    assert interp_even or B.call_counts(O, case, [p])[0] % 2 == 1


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def _buffer(dtype, nch, cap, oy, pad):
    """make_buffer's layout in numpy (the checker takes numpy arrays): these tests need nothing but numpy and never skip"""
    width = oy + cap + pad
    backing = np.full((nch + 2) * width * np.dtype(dtype).itemsize, B.POISON, dtype=np.uint8).view(dtype).reshape(nch + 2, width)
    return backing[1:1 + nch, oy:oy + cap], backing


def test_make_buffer_is_all_poison_and_its_view_sits_behind_the_guards():
    import torch
    for dtype in (np.float32, np.float64, np.complex64, np.complex128):
        nch, cap, oy, pad = 3, 11, 2, 3
        view, backing = B.make_buffer(torch, dtype, nch, cap, oy, pad, device="cpu")
        assert view.shape == (nch, cap) and backing.shape == (nch + 2, oy + cap + pad)
        assert view.data_ptr() - backing.data_ptr() == ((oy + cap + pad) + oy) * np.dtype(dtype).itemsize
        by, es = B.backing_bytes(backing)
        assert es == np.dtype(dtype).itemsize and (by == B.POISON).all()
        assert np.array_equal(by, B.backing_bytes(_buffer(dtype, nch, cap, oy, pad)[1])[0])
        view[:, :7] = 1.5
        B.assert_only_written(backing, nch, cap, oy, pad, 7, "torch backing")
        backing[0, 1] = 1.0
        with pytest.raises(AssertionError):
            B.assert_only_written(backing, nch, cap, oy, pad, 7, "torch backing, stray in the guard row")


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
def test_a_fully_written_interior_is_accepted_and_a_fresh_buffer_is_all_poison(dtype):
    nch, cap, oy, pad = 3, 11, 2, 3
    view, backing = _buffer(dtype, nch, cap, oy, pad)
    by, es = B.backing_bytes(backing)
    assert es == np.dtype(dtype).itemsize and (by == B.POISON).all()
    B.assert_only_written(backing, nch, cap, oy, pad, 0, "fresh")
    view[:, :7] = 1.5
    B.assert_only_written(backing, nch, cap, oy, pad, 7, "count < cap")
    view[:, :] = -2.0
    B.assert_only_written(backing, nch, cap, oy, pad, cap, "count == cap")


STRAYS = [
    # (name, count == cap?, (row, column) of the stray element relative to the view)
    ("one element behind the last output, count == cap", True, (1, "count")),
    ("one element behind the last output, count < cap", False, (1, "count")),
    ("one element behind the last output of the last row, count == cap", True, ("last", "count")),
    ("one element in front of a row's first", False, (0, -1)),
    ("one element in front of the last row's first, count == cap", True, (2, -1)),
    ("in the guard row above", False, (-1, 3)),
    ("in the guard row below", False, ("below", 0)),
]


@pytest.mark.parametrize("dtype", [np.float32, np.complex64, np.complex128])
@pytest.mark.parametrize("name,full,where", STRAYS, ids=[s[0] for s in STRAYS])
def test_a_stray_element_is_found_and_located(dtype, name, full, where):
    nch, cap, oy, pad = 3, 9, 1, 2
    count = cap if full else cap - 4
    view, backing = _buffer(dtype, nch, cap, oy, pad)
    view[:, :count] = 3.0
    B.assert_only_written(backing, nch, cap, oy, pad, count, name)
    row = {"last": nch - 1, "below": nch}.get(where[0], where[0])
    col = count if where[1] == "count" else where[1]
    backing[1 + row, oy + col] = 7.0                      # (through the backing store: the view cannot reach its guards)
    with pytest.raises(AssertionError) as ei:
        B.assert_only_written(backing, nch, cap, oy, pad, count, name)
    assert f"row {row}, column {col} of the view" in str(ei.value), str(ei.value)


def test_a_single_stray_byte_is_found():
    nch, cap, oy, pad = 2, 8, 1, 1
    for (row, col, byte) in ((0, 5, 0), (1, 8, 7), (-1, 0, 3), (2, 2, 6), (0, -1, 1)):
        view, backing = _buffer(np.complex64, nch, cap, oy, pad)
        view[:, :5] = 1.0
        raw = backing.reshape(-1).view(np.uint8).reshape(nch + 2, -1)
        raw[1 + row, (oy + col) * 8 + byte] ^= 0x01
        with pytest.raises(AssertionError) as ei:
            B.assert_only_written(backing, nch, cap, oy, pad, 5, "one byte")
        msg = str(ei.value)
        assert f"row {row}, column {col} of the view" in msg and f"byte {byte} of the element" in msg and "1 stray bytes" in msg, msg


def test_a_wrong_geometry_is_refused():
    view, backing = _buffer(np.float32, 2, 8, 1, 1)
    with pytest.raises(AssertionError):
        B.assert_only_written(backing, 2, 8, 1, 2, 4, "pad off by one")
    with pytest.raises(AssertionError):
        B.assert_only_written(backing, 2, 8, 1, 1, 9, "count > cap")


def test_row_strides_of_the_layouts():
    for es in (4, 8, 16):
        for cap in (100, 101, 102, 103):
            for name in B.layouts_for(es):
                oy = B.LAYOUTS[name][0]
                s = oy + cap + B.row_pad(name, oy, cap, es)
                if name == "tight":
                    assert s == cap
                elif name in ("A", "C"):
                    assert s % 2 == 1
                else:
                    assert s % 2 == 0 and (es != 4 or (s * es) % 16 != 0)
    assert {B.LAYOUTS[n][0] * 4 % 16 for n in B.layouts_for(4)} == {0, 4, 8, 12}
