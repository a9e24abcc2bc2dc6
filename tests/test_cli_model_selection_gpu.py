"""`ComputeMatches <yaml>` with SIFTmatch.model_selection : 1 on a mixed capture (synth.mixed_capture: facade images and 3-D-scene
images): the rows equal the Python matcher's and those of the host twin (MSFM_GEOMETRIC_VERIFICATION=host); facade pairs' rows equal
a verification_model : 2 run's and 3-D pairs' rows a verification_model : 0 run's; MSFM_CLI_TIMING=1 reports the choice; the invalid
combinations exit non-zero and write no rows."""
import os
import re
import shutil
import subprocess

import pytest

from monocularsfm_amd import _lib, database, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
EXE = os.path.join(HOST, "ComputeMatches")
N_FACADE, N_SCENE = 4, 4

YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : {mt}
SIFTmatch.verification_model : {model}
SIFTmatch.model_selection : {sel}
"""


@pytest.fixture(scope="module")
def exe(built_lib):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return EXE


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mixed") / "mixed.db")
    _, _, facade = synth.mixed_capture(N_FACADE, N_SCENE, n_desc=1500, seed=77, n_proto=5000, path=path)
    return path, facade


def rows(path):
    db = database.Database(path)
    r = db.db.execute("SELECT pair_id, rows, cols, data FROM matches ORDER BY pair_id").fetchall()
    db.Close()
    return r


def run(exe, cfg, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run([exe, str(cfg)], capture_output=True, text=True, env=env, timeout=600)


def cli(exe, capture, tmp_path, name, mt, model, sel, env=None, extra=""):
    path = str(tmp_path / (name + ".db"))
    shutil.copy(capture[0], path)
    cfg = tmp_path / (name + ".yaml")
    cfg.write_text(YAML.format(db=path, mt=mt, model=model, sel=sel) + extra)
    r = run(exe, cfg, env)
    return path, r


@pytest.mark.parametrize("mt", [0, 1])
def test_cli_rows(exe, capture, tmp_path, mt):
    from monocularsfm_amd.matcher import BruteFeatureMatcher, SequentialFeatureMatcher
    facade = capture[1]
    out = {}
    for name, model, sel, env in (("sel", 0, 1, {"MSFM_CLI_TIMING": "1"}), ("host", 0, 1, {"MSFM_GEOMETRIC_VERIFICATION": "host", "MSFM_CLI_TIMING": "1"}),
                                  ("f", 0, 0, {}), ("h", 2, 0, {})):
        path, r = cli(exe, capture, tmp_path, name, mt, model, sel, env)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = (rows(path), r)
    py = str(tmp_path / "py.db")
    shutil.copy(capture[0], py)
    cls = BruteFeatureMatcher if mt == 1 else SequentialFeatureMatcher
    with _lib.Context(0) as ctx:
        cls(py, ctx=ctx, verbose=False, geometric_verification="device", model_selection=True).RunMatching()
    sel_rows = out["sel"][0]
    assert sel_rows == rows(py) and sel_rows == out["host"][0]
    f_rows = {r[0]: r for r in out["f"][0]}
    h_rows = {r[0]: r for r in out["h"][0]}
    n_facade = n_scene = 0
    for r in sel_rows:
        i, j = _lib.pair_from_id(r[0])
        if facade[i] and facade[j]:
            assert r == h_rows[r[0]], (i, j)
            n_facade += 1
        elif not facade[i] and not facade[j]:
            assert r == f_rows[r[0]], (i, j)
            n_scene += 1
    assert n_facade >= 3 and n_scene >= 3, (n_facade, n_scene)
    assert sum(r[1] for r in sel_rows) > 500
    lines = []
    for name in ("sel", "host"):
        m = re.search(r"\[msfm two-view\] pairs verified (\d+) \| kept the homography's list (\d+)", out[name][1].stderr)
        assert m, out[name][1].stderr[-2000:]
        lines.append((int(m.group(1)), int(m.group(2))))
    assert lines[0] == lines[1] and lines[0][1] >= n_facade and lines[0][0] >= n_facade + n_scene, lines


@pytest.mark.parametrize("model,sel,extra,key", [(2, 1, "", "model_selection"),
                                                 (0, 1, "SIFTmatch.model_selection_h_ratio : 0\n", "model_selection_h_ratio"),
                                                 (0, 1, "SIFTmatch.model_selection_h_ratio : -0.5\n", "model_selection_h_ratio"),
                                                 (0, 1, "SIFTmatch.model_selection_h_ratio : nan\n", "model_selection_h_ratio"),
                                                 (0, 1, "SIFTmatch.model_selection_h_ratio : inf\n", "model_selection_h_ratio"),
                                                 (0, 2, "", "model_selection")])
def test_invalid_combinations_exit_non_zero(exe, capture, tmp_path, model, sel, extra, key):
    path, r = cli(exe, capture, tmp_path, "bad", 1, model, sel, extra=extra)
    assert r.returncode != 0 and key in r.stderr, r.stderr
    assert rows(path) == []
