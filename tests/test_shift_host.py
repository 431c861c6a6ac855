"""Random shift on the host: the numpy restatement tests/shift_np.py against np.pad + crop, the Philox draw's range, purity and
coverage, and the Python argument check of ReplayMemory.enable_random_shift (no GPU)."""
import numpy as np
import pytest

from tests import shift_np as S


def test_shift_images_is_edge_padding_plus_crop():
    rng = np.random.default_rng(0)
    H, W, C, pad = 7, 5, 6, 3
    x = rng.integers(0, 256, (1, H, W, C)).astype(np.float16)
    padded = np.pad(x[0], ((pad, pad), (pad, pad), (0, 0)), mode="edge")
    for dy in range(-pad, pad + 1):
        for dx in range(-pad, pad + 1):
            want = padded[pad + dy:pad + dy + H, pad + dx:pad + dx + W]
            got = S.shift_images(x, np.array([[dy, dx]]))[0]
            assert np.array_equal(got, want), (dy, dx)


def test_shift_images_keeps_trailing_axes():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, (3, 6, 4, 3, 1, 2)).astype(np.float16)
    sh = np.array([[1, -2], [0, 0], [-3, 3]])
    got = S.shift_images(x, sh)
    flat = S.shift_images(x.reshape(3, 6, 4, 6), sh).reshape(x.shape)
    assert np.array_equal(got, flat) and np.array_equal(got[1], x[1])


@pytest.mark.parametrize("pad", [1, 4, 16])
def test_shifts_stay_in_range(pad):
    s = S.shifts(12345, 7, 512, pad)
    assert s.shape == (2, 512, 2) and s.dtype == np.int32
    assert s.min() >= -pad and s.max() <= pad
    assert s.min() == -pad and s.max() == pad


def test_shifts_are_a_pure_function_of_seed_counter_row_and_column():
    a = S.shifts(3, 5, 64, 4)
    assert np.array_equal(a, S.shifts(3, 5, 64, 4))
    assert np.array_equal(a[:, :16], S.shifts(3, 5, 16, 4))           # (row b does not depend on B)
    assert not np.array_equal(a[0], a[1])                              # state_1 and state_2 draw differently
    assert not np.array_equal(a, S.shifts(3, 6, 64, 4))
    assert not np.array_equal(a, S.shifts(4, 5, 64, 4))
    assert not np.array_equal(S.shifts(3, 1 << 32, 64, 4), S.shifts(3, 0, 64, 4))      # (the counter's high word is keyed)
    assert not np.array_equal(S.shifts(1 << 32, 5, 64, 4), S.shifts(0, 5, 64, 4))      # (and the seed's)


def test_every_cell_occurs():
    pad, B = 4, 256
    seen = np.zeros((2, 2 * pad + 1, 2 * pad + 1), int)
    for n in range(64):
        s = S.shifts(0, n, B, pad)
        for which in (0, 1):
            np.add.at(seen[which], (s[which, :, 0] + pad, s[which, :, 1] + pad), 1)
    assert (seen > 0).all()
    # 16384 draws over 81 cells: ~202 each; a uniform draw stays well inside +-40 %
    assert seen.min() > 120 and seen.max() < 285, (seen.min(), seen.max())


def test_python_argument_check():
    from cartpoleplusplus_amd.replay_memory import check_random_shift
    assert check_random_shift((64, 48, 3, 2, 3), 4) == (64, 48, 4)
    assert check_random_shift((12, 10, 3, 1, 3), 0) == (12, 10, 0)
    assert check_random_shift((12, 10, 3, 1, 3), 9) == (12, 10, 9)
    for shape, pad in (((7,), 1), ((2, 2, 7), 1), ((64, 64, 3, 2, 3), -1), ((64, 64, 3, 2, 3), 17), ((12, 10, 3, 1, 3), 10),
                       ((12, 10, 3, 1, 3), 12), ((64, 64, 3, 2, 3), 1.5)):
        with pytest.raises(ValueError):
            check_random_shift(shape, pad)
