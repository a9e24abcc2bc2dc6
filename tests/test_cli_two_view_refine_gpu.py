"""`ComputeMatches <yaml>` with SIFTmatch.two_view_refine : 1 (under two_view_geometry : 1) on a synth.south_building_database: the
two_view_geometries table keeps its schema and holds the refined records -- the device executable (tv_refine_kernel) and the
host-RANSAC executable (RefineTwoView) write the same table, which differs from the table without the key; `matches` and stdout are
byte for byte what they are without the key; the key without two_view_geometry : 1, and bad optional keys, exit non-zero."""
import re

import pytest

from test_cli_two_view_geometry_gpu import base, copy_db, exe, run, tables  # noqa: F401  (module fixtures and helpers)

pytestmark = pytest.mark.gpu
REFINE = "SIFTmatch.two_view_min_num_inliers : 20\nSIFTmatch.two_view_refine : 1\n"


def strip(s):
    return re.sub(r"\t .*seconds.*\n|.*minutes.*\n|.*\[msfm.*\n", "", s)   # (the timing lines)


def test_refined_table_both_executables_and_nothing_else_changes(exe, base, tmp_path):   # noqa: F811
    src, _, _ = base
    off, dev, host = (copy_db(src, str(tmp_path / n)) for n in ("off.db", "dev.db", "host.db"))
    r_off, _, _ = run(exe, tmp_path, off, 1, extra="SIFTmatch.two_view_min_num_inliers : 20\n")
    r_dev, _, _ = run(exe, tmp_path, dev, 1, extra=REFINE)
    r_host, _, _ = run(exe, tmp_path, host, 1, env_extra={"MSFM_GEOMETRIC_VERIFICATION": "host"}, extra=REFINE)
    assert r_off.returncode == 0 and r_dev.returncode == 0 and r_host.returncode == 0, (r_off.stderr[-500:], r_dev.stderr[-500:], r_host.stderr[-500:])
    assert strip(r_dev.stdout) == strip(r_off.stdout) and r_dev.stdout.split("Elapsed")[0] == r_off.stdout.split("Elapsed")[0]
    m_off, g_off = tables(off)
    m_dev, g_dev = tables(dev)
    assert m_dev == m_off and len(m_dev) > 100
    assert tables(host) == (m_dev, g_dev)
    assert [r[0] for r in g_dev] == [r[0] for r in g_off] and g_dev != g_off
    changed = [a[9] != b[9] for a, b in zip(g_dev, g_off)]                               # the pose blob
    assert sum(changed) > 50
    for a, b, c in zip(g_dev, g_off, changed):
        assert a[1] == b[1] and a[2] == b[2] and a[3] >= b[3] and a[4] >= b[4]           # valid, n_kept; the counts do not drop
        assert c or a == b                                                                # an unrefined record: the same row


def test_key_without_the_two_view_geometry_exits_non_zero(exe, base, tmp_path):   # noqa: F811
    src, _, _ = base
    db = copy_db(src, str(tmp_path / "bad.db"))
    r, _, _ = run(exe, tmp_path, db, 0, extra="SIFTmatch.two_view_refine : 1\n")
    assert r.returncode != 0 and "SIFTmatch.two_view_refine" in r.stderr and "two_view_geometry : 1" in r.stderr
    assert tables(db) == ([], None)
    on = "SIFTmatch.two_view_refine : 1\n"
    for extra in (on + "SIFTmatch.two_view_refine_max_iters : 0\n", on + "SIFTmatch.two_view_refine_min_matches : 4\n",
                  on + "SIFTmatch.two_view_refine_step_tol : -1.0\n", "SIFTmatch.two_view_refine : 2\n"):
        r, _, _ = run(exe, tmp_path, db, 1, extra=extra)
        assert r.returncode != 0 and "two_view_refine" in r.stderr
    # the optional keys are checked only with the feature on: a stale one beside two_view_refine : 0 changes nothing
    plain, stale = copy_db(src, str(tmp_path / "plain.db")), copy_db(src, str(tmp_path / "stale.db"))
    r1, _, _ = run(exe, tmp_path, plain, 1)
    r2, _, _ = run(exe, tmp_path, stale, 1, extra="SIFTmatch.two_view_refine : 0\nSIFTmatch.two_view_refine_max_iters : 0\n")
    assert r1.returncode == 0 and r2.returncode == 0, r2.stderr[-500:]
    assert tables(stale) == tables(plain)
