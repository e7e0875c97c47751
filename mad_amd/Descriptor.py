"""Descriptor generation (hot path rows a9-a10).

Same constructor and entry point as the reference's `Descriptor`
(mad/Descriptor.py:14, :106): `Descriptor(subeqsp_size=16, dsc_radius=16,
dsc_size=64).generate_descriptors(ms, df_list)` fills `lin_ar_subeqsp` (int16[1024]) on
every oriented anchor and returns the list.  The arithmetic (step06,
Descriptor.py:123-202) runs in the HIP kernel `k_describe` through `mad_describe`.

MaD.run only ever constructs `Descriptor(dsc_radius=patch_size)` (MaD.py:362): 64 sub-cubes x 16 zones.  The constructor's other
options run on the device too and are pinned by goldens from the reference: `dsc_size` 27 / 8 / 1 (g17; built for the default
dsc_radius), `dsc_radius` 4 / 8 / 12 / 16 / 20 / 24 with 64 sub-cubes (g19 pins 20 and 24), and `subeqsp_size=112` -- the
reference's other EQSP table, rows of 64 x 112 = 7 168 counts (g18; default layout).  Rows whose counts exceed 127 (`dsc_size` 8
and 1 can) are described but refused by the int8 correlation (MAD_EDOM) rather than wrapped; at `dsc_radius` 24 (a sub-cube of
6^3 = 216 samples) they are matched exactly, as the rows of a wide set (include/mad_amd.h).
"""
import sys

import numpy as np

from . import _lib
from .eqsp.eqsp import EQSP_Sphere


class Descriptor(object):
    def __init__(self, subeqsp_size=16, dsc_radius=16, dsc_size=64):
        self.subeqsp_size = subeqsp_size
        self.subeqsp = EQSP_Sphere(size=subeqsp_size)
        self.cutoff_magn = 1e-12
        if dsc_radius % 2:
            print("MaD>> ERROR: radius %i invalid, must be even. Setting %i instead." % (dsc_radius, dsc_radius - 1))
            dsc_radius -= 1
        self.dsc_radius = dsc_radius // 2
        self.dsc_size = dsc_size
        if dsc_size not in (64, 27, 8, 1):
            print("MaD>> ERROR: invalid dsc size %i" % dsc_size)
            sys.exit(1)
        if subeqsp_size not in (16, 112):
            raise NotImplementedError("MaD> EQSP tables exist for 16 and 112 zones (eqsp.py:16): subeqsp_size=%r" % (subeqsp_size,))
        if subeqsp_size != 16 and (dsc_size != 64 or self.dsc_radius != 8):
            raise NotImplementedError("MaD> the 112-zone descriptor is built for the default layout (dsc_size 64, dsc_radius 16) only")
        if dsc_size != 64 and self.dsc_radius != 8:
            raise NotImplementedError("MaD> dsc_size 27, 8 and 1 are built for the default dsc_radius (16) only")
        dr = self.dsc_radius
        # sample lattices (Descriptor.py:34-35), kept for inspection
        self.dsc_layout = {
            0: np.rollaxis(np.array(np.mgrid[-2 * dr + 1:2 * dr + 1:2, -2 * dr + 1:2 * dr + 1:2, -2 * dr + 1:2 * dr + 1:2]), 0, 4),
            1: np.rollaxis(np.array(np.mgrid[-dr + 0.5:dr + 0.5, -dr + 0.5:dr + 0.5, -dr + 0.5:dr + 0.5]), 0, 4),
        }
        self.time6 = 0

    def _bind(self, lib):
        key = ("dsc", self.subeqsp_size)
        if lib._eq_loaded.get(1) != key:
            lib.set_eqsp(1, self.subeqsp.sphere_eqsp)
            lib._eq_loaded[1] = key

    def generate_descriptors(self, ms, df_list):
        print("MaD> Generating descriptors from %i oriented anchors..." % len(df_list))
        lib = _lib.get_lib()
        self._bind(lib)
        slots = ms.device_slots(lib)
        for octave in sorted(set(df.oct_scale for df in df_list)):
            ids = [i for i, df in enumerate(df_list) if df.oct_scale == octave]
            coords = np.array([df_list[i].coords for i in ids], dtype=np.int32).reshape(-1, 3)
            R = np.array([df_list[i].Rfinal for i in ids], dtype=np.float64).reshape(-1, 9)
            slot = slots[octave] if len(ms.grad_list) > 1 else slots[0]
            lattice = octave if len(ms.grad_list) > 1 else (1 if ms.oct_mode == "base" else 0)
            dsc = lib.describe(slot, lattice, coords, R, r=self.dsc_radius, Zd=self.subeqsp_size, dsc_size=self.dsc_size)
            for j, i in enumerate(ids):
                df = df_list[i]
                df.set_descriptor_info(self.subeqsp_size, self.dsc_radius)
                df.lin_ar_subeqsp = dsc[j].copy()
        return df_list

    def show_timing(self):
        print("MaD> Step timing: description runs on the GPU; use Lib.timing_get('describe')")
