"""Every lattice-allocating entry point of mad_fourier.hip gives back what it took: after a warm-up call of the same shapes (the
scratch buffers then exist) a second call leaves free device memory and the context's allocation count where they were.  Two
lattices (mode 0) and three (mode 1) for the scan and the search, N = 8 or 16 throughout."""
import numpy as np
import pytest

from mad_amd import fourier
from test_gpu_search import blobs, free_bytes, rotations, template

pytestmark = pytest.mark.gpu

O1, O2, OM = (0.0, 0.0, 0.0), (1.5, -3.0, 0.75), (-1.5, 0.0, 1.5)      # voxsp 1.5: whole and half voxels apart


def grid(shape, seed):
    return np.ascontiguousarray(blobs(shape, 6, seed, seed + 50), np.float32)


G1, G2, MASK = grid((13, 9, 16), 1), grid((11, 12, 10), 2), np.ascontiguousarray(np.clip(blobs((12, 12, 12), 8, 3), 0.0, 1.0), np.float32)
SMALL, TPL, BASE = grid((8, 7, 8), 4), template((3, 4, 2)), template((5, 5, 5))
SPECTRUM = np.fft.fftn(blobs((8, 8, 8), 4, 5, 55))
ROT, C0 = rotations(3), np.full(3, 2.0)

CALLS = {
    "map_fft": lambda lib: lib.map_fft(G1, O1, G2, O2, 1.5),
    "map_fft_one_grid": lambda lib: lib.map_fft(SMALL, O1),
    "map_fsc": lambda lib: lib.map_fsc(G1, O1, G2, O2, 1.5),
    "map_fsc_masked": lambda lib: lib.map_fsc_masked(G1, O1, G2, O2, 1.5, MASK, OM, shell_r=3, seed=11),
    "map_phase_randomize": lambda lib: lib.map_phase_randomize(SPECTRUM, 2, seed=11),
    "map_filter": lambda lib: lib.map_filter(G1, np.ones(fourier.gain_len(fourier.filter_lattice(G1.shape, 0, G2.shape))), 0, G2),
    "map_ifft": lambda lib: lib.map_ifft(SPECTRUM),
    "map_scan_mode0": lambda lib: lib.map_scan(G1, [TPL, TPL[::-1].copy()], 0.05, 0.0, 0, 0.0, 5),
    "map_scan_mode1": lambda lib: lib.map_scan(G1, [TPL, TPL[::-1].copy()], 0.05, 0.0, 1, 0.0, 5),
    "map_search_mode0": lambda lib: lib.map_search(SMALL, BASE, C0, 5, ROT, 0.05, 0.0, 0, 0.0, 5),
    "map_search_mode1": lambda lib: lib.map_search(SMALL, BASE, C0, 5, ROT, 0.05, 0.0, 1, 0.0, 5),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_second_call_leaves_device_memory_as_it_found_it(lib, name):
    call = CALLS[name]
    first = call(lib)      # the scratch buffers of these shapes exist from here on
    lib.synchronize()
    free0, allocs0 = free_bytes(lib), lib.device_allocations()
    again = call(lib)
    lib.synchronize()
    assert lib.device_allocations() == allocs0 and free_bytes(lib) == free0
    for a, b in zip(first if isinstance(first, tuple) else (first,), again if isinstance(again, tuple) else (again,)):
        assert np.array_equal(a, b)
