"""`fourier.Scan` and `fourier.Search` turn a peak into a placement, and `Dmap.scan` / `Dmap.search` refuse bad arguments under their own
names before any library call.  Every expected number is a literal: small integer origins, spacings and rotations.  No device."""
import numpy as np
import pytest

from mad_amd import _lib, fourier, mapio
from mad_amd.Dmap import Dmap

ORIGIN, VOXSP, CENTROID = (10.0, 20.0, 30.0), 2.0, (1.0, 2.0, 3.0)
ROT = np.array([np.eye(3), [[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])      # the identity and a quarter turn about z
PEAKS = np.array([[1, 2, 3, 0.75, 1], [0, 0, 5, 0.5, 0], [4, 1, 0, 0.25, 1]], np.float64)
BEST = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
ATOMS = np.array([[2.0, 2.0, 3.0], [1.0, 4.0, 3.0]])
TURNED = np.array([[1.0, 3.0, 3.0], [-1.0, 2.0, 3.0]])      # (ATOMS - CENTROID) @ ROT[1] + CENTROID


def scan():
    return fourier.Scan(BEST, np.zeros(BEST.shape, np.int32), PEAKS, 7, ORIGIN, VOXSP, ROT, CENTROID, [[4.0, 6.0, 8.0], [-2.0, 0.0, 2.0]], N=8,
                        e_min=0.5, mode=1)


def search():
    return fourier.Search(BEST, np.zeros(BEST.shape, np.int32), PEAKS, 7, 2, ORIGIN, VOXSP, ROT, CENTROID, 5, N=8, e_fill=0.5, mode=1)


# T of the three peaks: Scan origin + u voxsp - template_origins[rotation]; Search origin + (u + 2) voxsp - centroid
CASES = [(scan, [(14.0, 24.0, 34.0), (6.0, 14.0, 32.0), (20.0, 22.0, 28.0)], ORIGIN),
         (search, [(15.0, 26.0, 37.0), (13.0, 22.0, 41.0), (21.0, 24.0, 31.0)], (14.0, 24.0, 34.0))]
IDS = ["scan", "search"]


class Atoms(object):
    """What `place` needs of a PDB."""

    def __init__(self, coords):
        self.coords, self.tag = np.array(coords, np.float64), ["kept"]

    def get_coords(self):
        return self.coords

    def set_coords(self, c):
        self.coords = np.asarray(c, np.float64)


@pytest.mark.parametrize("make, shifts, write_origin", CASES, ids=IDS)
def test_attributes_and_pose(make, shifts, write_origin):
    r = make()
    assert r.best is BEST and r.n_found == 7 and r.voxsp == 2.0 and (r.N, r.mode) == (8, 1)
    assert r.peaks.shape == (3, 5) and r.rotations.shape == (2, 3, 3)
    assert np.array_equal(r.origin, ORIGIN) and np.array_equal(r.centroid, CENTROID)
    if make is scan:
        assert r.best_t.shape == BEST.shape and r.e_min == 0.5 and r.template_origins.shape == (2, 3)
    else:
        assert r.best_r.shape == BEST.shape and r.e_fill == 0.5 and (r.n_skipped, r.edge) == (2, 5)
    for i, (j, score) in enumerate(((1, 0.75), (0, 0.5), (1, 0.25))):
        got_j, R, T, got_score = r.pose(i)
        assert (got_j, got_score) == (j, score) and type(got_j) is int and type(got_score) is float
        assert np.array_equal(R, ROT[j]) and np.array_equal(T, shifts[i])


@pytest.mark.parametrize("make, shifts, write_origin", CASES, ids=IDS)
def test_place_moves_a_copy(make, shifts, write_origin):
    r = make()
    want0, want1 = TURNED + np.array(shifts[0]), ATOMS + np.array(shifts[1])
    assert np.array_equal(r.place(0, ATOMS), want0) and np.array_equal(r.place(1, ATOMS), want1)
    assert np.array_equal(r.place(0, ATOMS.tolist()), want0)
    pdb = Atoms(ATOMS)
    out = r.place(0, pdb)
    assert out is not pdb and isinstance(out, Atoms) and out.tag == ["kept"] and out.tag is not pdb.tag
    assert np.array_equal(out.get_coords(), want0) and np.array_equal(pdb.get_coords(), ATOMS)


@pytest.mark.parametrize("make, shifts, write_origin", CASES, ids=IDS)
def test_write_peaks_text(make, shifts, write_origin, tmp_path):
    path = tmp_path / "peaks.csv"
    make().write_peaks(str(path))
    rows = ["0,1,2,3,0.75,1", "1,0,0,5,0.5,0", "2,4,1,0,0.25,1"]
    want = "rank,ux,uy,uz,score,rotation,tx,ty,tz\n" + "".join("%s,%.6f,%.6f,%.6f\n" % ((row,) + T) for row, T in zip(rows, shifts))
    assert path.read_text() == want
    if make is scan:
        assert want.splitlines()[1] == "0,1,2,3,0.75,1,14.000000,24.000000,34.000000"
    else:
        assert want.splitlines()[3] == "2,4,1,0,0.25,1,21.000000,24.000000,31.000000"


@pytest.mark.parametrize("make, shifts, write_origin", CASES, ids=IDS)
def test_write_passes_the_volume_and_its_origin(make, shifts, write_origin, monkeypatch):
    calls = []
    monkeypatch.setattr(mapio, "write_volume", lambda *a: calls.append(a))
    make().write("scores.mrc")
    (name, vol, origin, voxsp), = calls
    assert name == "scores.mrc" and vol.dtype == np.float32 and np.array_equal(vol, BEST)
    assert isinstance(origin, tuple) and origin == write_origin and voxsp == 2.0


# ---------------------------------------------------------------------------
# the front ends' refusals, before any library call
# ---------------------------------------------------------------------------

def dmap():
    d = Dmap.__new__(Dmap)
    d.grid3d = np.ones((8, 8, 8), np.float32)
    d.voxsp = 1.0
    d.xi = d.yi = d.zi = 0.0
    d.xb = d.yb = d.zb = 8
    return d


BAD = [(dict(mode="both"), "mode 'both'"), (dict(mode=1), "mode 1"),
       (dict(resolution=0.0), "resolution 0.0"), (dict(resolution=-3.0), "resolution -3.0"), (dict(resolution=float("nan")), "resolution nan"),
       (dict(resolution=float("inf")), "resolution inf"), (dict(resolution=None), "resolution None"),
       (dict(isovalue=float("inf")), "isovalue inf"), (dict(isovalue=float("nan")), "isovalue nan"),
       (dict(min_fill=-0.5), "min_fill -0.5"), (dict(min_fill=float("nan")), "min_fill nan"),
       (dict(structure=np.zeros((0, 3))), "no atoms"), (dict(structure=[]), "no atoms"),
       (dict(rotations=np.eye(3)), "rotations of shape (3, 3)"), (dict(rotations=np.zeros((0, 3, 3))), "rotations of shape (0, 3, 3)"),
       (dict(rotations=np.zeros((2, 3, 2))), "rotations of shape (2, 3, 2)")]


@pytest.mark.parametrize("method", ("scan", "search"))
@pytest.mark.parametrize("kw, text", BAD, ids=[t for _, t in BAD])
def test_front_end_refuses_under_its_own_name(method, kw, text, monkeypatch):
    def no_device():
        raise AssertionError("the library was asked for before the arguments were refused")
    monkeypatch.setattr(_lib, "get_lib", no_device)
    args = dict(structure=ATOMS, resolution=8.0)
    args.update(kw)
    with pytest.raises(ValueError) as err:
        getattr(dmap(), method)(**args)
    msg = str(err.value)
    assert msg.startswith("Dmap.%s: " % method) and text in msg, msg
