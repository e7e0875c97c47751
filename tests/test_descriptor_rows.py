"""DescriptorRows on the host (a stub stands in for the device set): the descriptor cache written from `arrays()` is the file a list
of DensityFeature rows gives, and `_load_descriptors` -> `arrays()` round-trips it."""
import numpy as np

from mad_amd.DensityFeature import DensityFeature
from mad_amd.rows import DescriptorRows


class StubSet(object):
    """What DescriptorRows reads of a DeviceSet: size() and one download()."""

    def __init__(self, host):
        self.host = host
        self.downloads = 0

    def size(self):
        return len(self.host["anchor"]), 0

    def download(self, want_dsc=True, D=1024):
        self.downloads += 1
        return self.host


def _fixture(seed=7):
    """Anchors as the detector lists them (the last one repeats the coordinates of the first) and rows as orientation +
    description order them: anchor order x main x sec."""
    rng = np.random.default_rng(seed)
    n_anc = 6
    coords = rng.integers(10, 60, (n_anc, 3)).astype(np.int64)
    octave = np.array([0, 0, 1, 1, 1, 0])
    coords[-1] = coords[0]
    octave[-1] = octave[0]
    vs = np.where(octave == 0, 0.6, 1.2)[:, None]
    map_coords = coords * vs + np.array([-3.0, 1.5, 2.25])
    subv = map_coords + rng.normal(scale=0.2, size=(n_anc, 3))
    subv[-1] = subv[0]
    index = np.arange(n_anc)
    anchor, main, sec = [], [], []
    for a in (0, 1, 3, 4, 5):      # anchor 2 was refused by the orientation
        for mb in sorted(rng.choice(112, size=int(rng.integers(1, 3)), replace=False)):
            for sb in sorted(rng.choice(6, size=int(rng.integers(1, 3)), replace=False)):
                anchor.append(a)
                main.append(int(mb))
                sec.append(int(sb))
    n = len(anchor)
    host = dict(anchor=np.array(anchor, np.int32), main=np.array(main, np.int32), sec=np.array(sec, np.int32),
                R=rng.normal(size=(n, 3, 3)), dsc=rng.integers(0, 64, (n, 1024)).astype(np.int16))
    rows = []
    for r in range(n):
        a = anchor[r]
        df = DensityFeature()
        df.set_detector_info(int(index[a]), int(octave[a]), [coords[a, 0], coords[a, 1], coords[a, 2]], map_coords[a], subv[a], 0.5)
        df.set_orientator_info(112, 8)
        df.main_bin, df.sec_bin, df.Rfinal = main[r], sec[r], host["R"][r].copy()
        df.set_descriptor_info(16, 8)
        df.lin_ar_subeqsp = host["dsc"][r].copy()
        rows.append(df)
    stub = StubSet(host)
    dr = DescriptorRows.built(stub, index, octave, coords, map_coords, subv, eqsp_size=112, subeqsp_size=16, D=1024)
    return dr, rows, stub


def _npz(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def test_cache_from_arrays_is_the_cache_from_rows(tmp_path, monkeypatch):
    from mad_amd import MaD as M
    monkeypatch.setattr(M, "h5py", None)
    dr, rows, stub = _fixture()
    m = M.MaD()
    m._save_descriptors(rows, str(tmp_path / "a.h5"))
    m._save_descriptors(dr, str(tmp_path / "b.h5"))
    assert stub.downloads == 1
    a, b = _npz(tmp_path / "a.npz"), _npz(tmp_path / "b.npz")
    assert sorted(a) == sorted(b) == ["coords", "dsc", "info", "rot"]
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # the rows it materialises (from the same one download) carry the stage path's fields
    assert len(dr) == len(rows)
    for x, y in zip(rows, dr):
        for f in ("index", "oct_scale", "main_bin", "sec_bin", "eqsp_size", "subeqsp_size"):
            assert getattr(x, f) == getattr(y, f), f
        for f in ("coords", "map_coords", "subv_map_coords", "Rfinal", "lin_ar_subeqsp"):
            np.testing.assert_array_equal(np.asarray(getattr(x, f), np.float64), np.asarray(getattr(y, f), np.float64), err_msg=f)
    assert stub.downloads == 1


def test_load_descriptors_round_trips_through_arrays(tmp_path, monkeypatch):
    from mad_amd import MaD as M
    monkeypatch.setattr(M, "h5py", None)
    monkeypatch.delenv("MAD_STAGE_PATH", raising=False)
    dr, rows, _ = _fixture(3)
    m = M.MaD()
    name = str(tmp_path / "x.h5")
    m._save_descriptors(dr, name)
    back = m._load_descriptors(name)
    assert isinstance(back, DescriptorRows) and len(back) == len(rows)
    ref, got = dr.arrays(), back.arrays()
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)
    # the set a loaded cache becomes: anchors = the unique sub-voxel positions in np.unique order, one per repeated position
    subv = ref["coords"][:, 2]
    np.testing.assert_array_equal(back.anchor_subv, np.unique(subv, axis=0))
    assert [x.main_bin for x in back] == [x.main_bin for x in rows]
    # the stage path keeps its list of rows
    monkeypatch.setenv("MAD_STAGE_PATH", "1")
    listed = m._load_descriptors(name)
    assert isinstance(listed, list) and len(listed) == len(rows)
    np.testing.assert_array_equal(np.array([x.lin_ar_subeqsp for x in listed]), ref["dsc"])


def test_empty_rows_write_the_empty_cache(tmp_path, monkeypatch):
    from mad_amd import MaD as M
    monkeypatch.setattr(M, "h5py", None)
    stub = StubSet(dict(anchor=np.zeros(0, np.int32), main=np.zeros(0, np.int32), sec=np.zeros(0, np.int32), R=np.zeros((0, 3, 3)),
                        dsc=np.zeros((0, 1024), np.int16)))
    dr = DescriptorRows.built(stub, [], [], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    m = M.MaD()
    m._save_descriptors([], str(tmp_path / "a.h5"))
    m._save_descriptors(dr, str(tmp_path / "b.h5"))
    a, b = _npz(tmp_path / "a.npz"), _npz(tmp_path / "b.npz")
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
    assert len(m._load_descriptors(str(tmp_path / "b.h5"))) == 0
