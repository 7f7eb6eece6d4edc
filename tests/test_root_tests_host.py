"""Host side of the root tests (no GPU): elw_confidence_set on hand-made vectors, and that the
new entry points exist."""
import os
import subprocess

import numpy as np
import pytest

import root_digger_amd as rd
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RD = os.path.join(ROOT, "root_digger_amd", "bin", "rd_amd")


def test_rd_amd_refuses_root_tests_without_rell(tmp_path):
    """decided from the options alone, before any device is touched"""
    prefix = str(tmp_path / "no")
    for extra in ([], ["--site-lh"]):
        out = subprocess.run([RD, "--msa", os.path.join(util.DATA, "10.fasta"), "--tree", os.path.join(util.DATA, "10.tree"),
                              "--exhaustive", "--silent", "--prefix", prefix, "--root-tests"] + extra,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode != 0
        assert "--root-tests: " in out.stdout and "--rell" in out.stdout
    assert not os.path.exists(prefix + ".roottests.tsv") and not os.path.exists(prefix + ".ckp")


def test_the_library_exports_the_new_calls():
    assert hasattr(rd.lib, "rdamd_rell_tests") and hasattr(rd.lib, "rdamd_rell_last_tests_ms")
    assert rd.rell_last_tests_ms() >= 0.0


def test_elw_confidence_set_takes_rows_by_decreasing_weight():
    elw = np.array([0.05, 0.5, 0.02, 0.3, 0.13])
    assert rd.elw_confidence_set(elw, 0.9).tolist() == [False, True, False, True, True]      # 0.93
    assert rd.elw_confidence_set(elw).tolist() == [True, True, False, True, True]            # 0.93 < 0.95 <= 0.98
    assert rd.elw_confidence_set(elw, 0.99).tolist() == [True, True, True, True, True]
    assert rd.elw_confidence_set(elw, 0.5).tolist() == [False, True, False, False, False]
    assert rd.elw_confidence_set(elw, 0.51).tolist() == [False, True, False, True, False]
    assert rd.elw_confidence_set(elw).dtype == np.bool_


def test_elw_confidence_set_orders_ties_by_index():
    elw = np.array([0.25, 0.25, 0.25, 0.25])
    assert rd.elw_confidence_set(elw, 0.5).tolist() == [True, True, False, False]
    assert rd.elw_confidence_set(elw, 0.6).tolist() == [True, True, True, False]
    assert rd.elw_confidence_set(np.array([0.1, 0.4, 0.1, 0.4]), 0.85).tolist() == [True, True, False, True]


def test_elw_confidence_set_stops_where_the_level_is_reached_exactly():
    # binary fractions: the running sums are exact
    elw = np.array([0.125, 0.5, 0.25, 0.125])
    assert rd.elw_confidence_set(elw, 0.75).tolist() == [False, True, True, False]
    assert rd.elw_confidence_set(elw, 0.875).tolist() == [True, True, True, False]
    assert rd.elw_confidence_set(elw, 0.8750001).tolist() == [True, True, True, True]


def test_elw_confidence_set_at_level_one_and_on_one_row():
    elw = np.array([0.125, 0.5, 0.25, 0.125])
    assert rd.elw_confidence_set(elw, 1.0).tolist() == [True, True, True, True]
    assert rd.elw_confidence_set(np.array([0.5, 0.5, 0.0]), 1.0).tolist() == [True, True, False]
    assert rd.elw_confidence_set(np.array([1.0])).tolist() == [True]
    assert rd.elw_confidence_set(np.array([1.0]), 1.0).tolist() == [True]
    # weights that fall short of the level by rounding: every row, no error
    assert rd.elw_confidence_set(np.array([0.3, 0.3, 0.3]), 0.95).tolist() == [True, True, True]
    with pytest.raises(ValueError):
        rd.elw_confidence_set(np.ones((2, 2)))
