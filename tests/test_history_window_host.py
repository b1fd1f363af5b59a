"""engine.ring_window: the default window of the four history readers
(catchment_series, band_series, coarse_series, cell_aggregate), without a GPU."""

from __future__ import annotations

import numpy as np

from topoflow_glacier.engine import ring_window


def test_default_window_is_the_last_steps_in_step_order():
    assert ring_window(0, 8, None, None) == (0, 1)    # before the first step: slot 0 alone
    assert ring_window(5, 8, None, None) == (0, 5)    # the ring has not wrapped
    assert ring_window(13, 8, None, None) == (5, 8)   # step 5 is the oldest of the eight still held
    assert ring_window(8, 8, None, None) == (0, 8)
    first, count = ring_window(13, 8, None, 3)        # steps 10, 11, 12
    assert (first, count) == (2, 3)


def test_explicit_values_pass_through():
    assert ring_window(13, 8, 6, None) == (6, 8)      # an explicit first keeps the default count
    assert ring_window(13, 8, 6, 2) == (6, 2)
    assert ring_window(0, 8, 3, None) == (3, 1)
    # out-of-range values are the library's to reject, not this function's to mend
    assert ring_window(13, 8, None, 0)[1] == 0
    assert ring_window(13, 8, None, -2)[1] == -2
    assert ring_window(13, 8, -1, 0) == (-1, 0)
    assert ring_window(13, 8, 9, 20) == (9, 20)


def test_numpy_integers_come_back_as_int():
    for args in ((np.int64(13), np.int32(8), None, None), (13, 8, np.int64(6), np.int32(2)),
                 (np.int64(0), np.int64(8), None, None), (np.int32(13), 8, None, np.int64(3))):
        first, count = ring_window(*args)
        assert type(first) is int and type(count) is int, args
    assert ring_window(np.int64(13), np.int32(8), None, None) == (5, 8)
    assert ring_window(np.int32(13), 8, None, np.int64(3)) == (2, 3)
