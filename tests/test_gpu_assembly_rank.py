"""MaD.build_assembly end to end through the device heads (mad_rank_copies / mad_rank_models) against the same run with
MAD_ASSEMBLY_HOST=1 (the host loops): every file written, stdout and complex_ranking.csv byte for byte, on a synthetic
homo-hexamer and a three-subunit heteromer whose solutions partly overlap and partly lie far apart."""
import os

import numpy as np
import pytest

from mad_amd import _lib, synth


@pytest.fixture()
def default_lib(lib):
    old = _lib._default
    _lib._default = lib
    yield lib
    _lib._default = old


def _solutions(folder, key, seed, sites, counts, jitter=2.5):
    """counts[s] solutions of one subunit around sites[s]: the same globule, the same rotation, centres `jitter` A apart at most
    per axis -- solutions of one site overlap heavily, solutions of different sites barely or not at all."""
    rng = np.random.default_rng(seed)
    coords, names, elems = synth.random_globule(110, 8.0, seed)
    files, placed = [], []
    for site, cnt in zip(sites, counts):
        R = synth.random_rotation(rng)
        for _ in range(cnt):
            c = synth.place(coords, R, np.asarray(site, float) + rng.uniform(-jitter, jitter, 3))
            files.append(os.path.join(folder, "sol_%s_%d.pdb" % (key, len(files))))
            synth.write_pdb(files[-1], c, names, elems)
            placed.append(c)
    return files, placed, synth.masses(elems)


def _run(lib, tmp_path, tag, subunits, placed, mass, host, monkeypatch, capsys):
    from mad_amd.MaD import MaD
    grid, x0, y0, z0 = lib.structure_to_density(np.concatenate(placed), np.concatenate(mass), 8.0, 2.0, pad=4)
    map_sit = str(tmp_path / "map.sit")
    synth.write_situs(map_sit, grid, (x0, y0, z0), 2.0)
    m = MaD()
    m.out_folder = str(tmp_path / ("out_%s_%s" % (tag, "host" if host else "device")))
    os.makedirs(m.out_folder)
    m.processed_map, m.map_name, m.resolution = map_sit, "synthetic", 8.0
    m.buildable_subunits = subunits
    if host:
        monkeypatch.setenv("MAD_ASSEMBLY_HOST", "1")
    else:
        monkeypatch.delenv("MAD_ASSEMBLY_HOST", raising=False)
    capsys.readouterr()
    calls = []
    for name in ("rank_copies", "rank_models"):      # count the device calls of this run
        def counted(*a, _f=getattr(lib, name), **kw):
            calls.append(1)
            return _f(*a, **kw)
        monkeypatch.setattr(lib, name, counted)
    m.build_assembly()
    monkeypatch.undo()
    out = capsys.readouterr().out
    files = {}
    for base, _, names in os.walk(m.out_folder):
        for nm in names:
            with open(os.path.join(base, nm), "rb") as fh:
                files[os.path.relpath(os.path.join(base, nm), m.out_folder)] = fh.read()
    return out, files, len(calls)


def _compare(lib, tmp_path, tag, subunits, placed, mass, monkeypatch, capsys, want_calls):
    dev = _run(lib, tmp_path, tag, subunits, placed, mass, False, monkeypatch, capsys)
    host = _run(lib, tmp_path, tag, subunits, placed, mass, True, monkeypatch, capsys)
    assert dev[2] == want_calls and host[2] == 0
    assert "on the host" not in dev[0]
    assert dev[0] == host[0]
    assert sorted(dev[1]) == sorted(host[1]) and "complex_ranking.csv" in dev[1]
    for name in dev[1]:
        assert dev[1][name] == host[1][name], name
    return dev


@pytest.mark.gpu
def test_homo_hexamer(default_lib, tmp_path, monkeypatch, capsys):
    ring = [(17.0 * np.cos(a), 17.0 * np.sin(a), 0.0) for a in np.arange(6) * np.pi / 3]
    sites = ring + [(0.0, 0.0, 70.0), (60.0, 0.0, -50.0)]
    files, placed, mass = _solutions(str(tmp_path), "A", 5, sites, [2, 2, 2, 2, 1, 1, 2, 2])      # 14 solutions
    out, written, _ = _compare(default_lib, tmp_path, "homo", {"A": [6, files]}, placed[:12], [mass] * 12, monkeypatch, capsys, 1)
    models = [n for n in written if n.startswith("assembly_models")]
    assert 1 <= len(models) <= 10 and "MaD> Assembling 6 copies of chain A from 14 solutions..." in out


@pytest.mark.gpu
def test_three_subunit_heteromer(default_lib, tmp_path, monkeypatch, capsys):
    fa, pa, ma = _solutions(str(tmp_path), "A", 7, [(-20.0, 0.0, 0.0), (20.0, 0.0, 0.0)], [9, 3])
    fb, pb, mb = _solutions(str(tmp_path), "B", 8, [(0.0, 22.0, 0.0), (0.0, 80.0, 40.0), (0.0, 0.0, 8.0)], [5, 4, 3])
    fc, pc, mc = _solutions(str(tmp_path), "C", 9, [(0.0, -22.0, 0.0), (0.0, -10.0, 24.0), (90.0, 90.0, 0.0)], [8, 3, 2])
    subunits = {"A": [2, fa], "B": [1, fb], "C": [2, fc]}
    placed = [pa[0], pa[9], pb[0], pc[0], pc[8]]
    mass = [ma, ma, mb, mc, mc]
    out, written, _ = _compare(default_lib, tmp_path, "hetero", subunits, placed, mass, monkeypatch, capsys, 3)
    subs = [n for n in written if n.startswith("subcomplexes")]
    assert 12 < len(subs) <= _lib.RANK_MAX_N      # B's 12 single solutions and the clash-free pairs of A and of C
    assert any(n.startswith("assembly_models") for n in written) and "MaD> Building assembly models from 3 components..." in out
