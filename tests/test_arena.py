"""The sentinel arena (tests/arena.py) can fail: stray writes planted into a CPU arena are found and named by region,
row, column and side; a run that writes exactly the owned bytes passes."""
import pytest
import torch

from tests.arena import FILL, MIN_GUARD, Arena


def carved():
    """A pitched double matrix at an 8-byte offset, a status matrix at offset 1, a dense status matrix at offset 0."""
    a = Arena("cpu", 1 << 16)
    pred = a.carve(5, 3, 7, torch.float64, 8, name="pred")
    st1 = a.carve(4, 6, 6, torch.uint8, 1, name="status1")
    st0 = a.carve(4, 8, 8, torch.uint8, 0, name="status0")
    return a, pred, st1, st0


def start_of(a, name):
    return next(r for r in a.regions if r.name == name)


def test_views_sit_where_they_were_asked_to_and_are_dirty_on_entry():
    a, pred, st1, st0 = carved()
    base = a.buf.data_ptr()
    assert base % 256 == 0
    assert (pred.data_ptr() - base) % 256 == 8 and pred.stride() == (7, 1) and pred.shape == (5, 3)
    assert (st1.data_ptr() - base) % 256 == 1 and (st0.data_ptr() - base) % 256 == 0
    assert (st1 == FILL).all() and (st0 == FILL).all()
    assert (pred.view(torch.int64) == -0x5A5A5A5A5A5A5A5B).all()  # 0xA5A5... as a signed 64-bit integer
    assert torch.isfinite(pred).all() and (pred < 0).all() and (pred.abs() < 1e-100).all()
    regs = sorted(a.regions, key=lambda r: r.start)
    assert regs[0].start >= MIN_GUARD and a.n_bytes - regs[-1].end >= MIN_GUARD
    for lo, hi in zip(regs, regs[1:]):
        assert hi.start - lo.end >= MIN_GUARD
    a.assert_clean()


def test_a_run_that_writes_exactly_the_owned_bytes_passes():
    a, pred, st1, st0 = carved()
    pred[:] = 1.5
    st1[:] = 0
    st0[:] = 3
    a.assert_clean()
    wide = a.carve(3, 2, 1000, torch.float64, 0, name="wide")  # guards grow with the pitch: a store one row off stays inside
    r = start_of(a, "wide")
    assert r.guard == 8000 and a.n_bytes - r.end >= 8000
    wide[:] = 0.0
    a.assert_clean()
    a.carve(2, 4, 4, torch.uint8, 0, name="behind_wide")  # the gap behind a wide pitch is the wide region's guard
    assert start_of(a, "behind_wide").start - r.end >= 8000


def planted(a, off, n):
    a.buf[off:off + n] = 0
    with pytest.raises(AssertionError) as e:
        a.assert_clean()
    return str(e.value)


def test_eight_bytes_after_a_rows_last_column_are_named_as_padding_of_that_row():
    a, pred, _, _ = carved()
    r = start_of(a, "pred")
    msg = planted(a, r.start + 2 * r.pitch + 3 * 8, 8)  # row 2, column 3 = the first padding element
    assert "8 byte(s) outside" in msg
    assert "first: " in msg and "region 'pred'" in msg and "row 2, column 3, byte 0" in msg and "padding" in msg
    assert "last: " in msg and "row 2, column 3, byte 7" in msg


def test_eight_bytes_before_the_first_element():
    a, _, _, _ = carved()
    r = start_of(a, "pred")
    msg = planted(a, r.start - 8, 8)
    assert "region 'pred'" in msg and "before the first row, 8 byte(s) in front of element [0, 0]" in msg
    assert "before the first row, 1 byte(s) in front" in msg  # the last offending byte


def test_eight_bytes_after_the_last_rows_last_column():
    a, _, _, _ = carved()
    r = start_of(a, "pred")
    assert r.end == r.start + (4 * 7 + 3) * 8  # the last row owns cols elements, not ld
    msg = planted(a, r.end, 8)
    assert "region 'pred'" in msg and "after the last row, 0 byte(s) past the last column of row 4" in msg
    assert "after the last row, 7 byte(s) past" in msg


def test_one_byte_after_a_status_region():
    a, _, _, _ = carved()
    r = start_of(a, "status0")
    msg = planted(a, r.end, 1)
    assert "1 byte(s) outside" in msg and "region 'status0'" in msg and "after the last row, 0 byte(s) past" in msg


def test_one_byte_into_the_gap_in_front_of_a_status_region_at_offset_one():
    a, _, _, _ = carved()
    r = start_of(a, "status1")
    assert r.start % 256 == 1
    msg = planted(a, r.start - 1, 1)  # the byte an aligned 8-byte clear of the first row would hit
    assert "region 'status1'" in msg and "before the first row, 1 byte(s) in front of element [0, 0]" in msg


def test_reset_refills_and_forgets():
    a, pred, _, _ = carved()
    pred[:] = 2.0
    a.buf[10] = 0
    a.reset()
    assert (a.buf == FILL).all() and not a.regions and not a.owned.any()
    a.assert_clean()
