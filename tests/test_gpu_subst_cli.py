"""`rd_amd --exhaustive --substitutions` on the 10-taxon fixture: the rows of
<prefix>.substitutions.tsv and <prefix>.mutations.tsv against Model.substitutions at the best
record's root and parameters, the branch names against <prefix>.substitutions.tree, and every other
output file byte for byte against a run without the option."""
import os
import re
import subprocess

import numpy as np
import pytest

import root_digger_amd as rd
import util
from test_gpu_brlen import MSA, TREE

pytestmark = pytest.mark.gpu

NEW = [".mutations.tsv", ".substitutions.tree", ".substitutions.tsv"]


def _run(args):
    return subprocess.run([os.path.join(util.ROOT, "root_digger_amd", "bin", "rd_amd")] + args, capture_output=True, text=True,
                          timeout=600)


def test_rd_amd_substitutions(tmp_path):
    ref = os.path.join(util.ROOT, "oracle", "_ref", "liblbfgsb_ref.so")
    common = ["--msa", MSA, "--tree", TREE, "--exhaustive", "--silent", "--rate-cats", "4",
              "--atol", "1e-3", "--brtol", "1e-3", "--bfgstol", "1e-3", "--factor", "1e12", "--seed", "5"]
    if os.path.exists(ref):
        common += ["--lbfgsb", ref]
    prefix, plain = str(tmp_path / "subst"), str(tmp_path / "plain")
    min_prob = 0.3
    out = _run(common + ["--prefix", prefix, "--substitutions", "--subst-min-prob", str(min_prob)])
    assert out.returncode == 0, out.stdout + out.stderr
    records = rd.Checkpoint(prefix).read_results()
    best = max(range(len(records)), key=lambda i: (records[i][1], -i))   # the first maximum
    tree = rd.Tree.from_file(TREE)
    m = rd.Model.from_file(tree, MSA, rate_cats=4, seed=5)
    m.initialize_partitions()
    rl = tree.root_location(records[best][0]).with_ratio(records[best][2])
    want = m.substitutions(rl, records[best][3])
    weights, pattern_of = m.site_patterns()
    n, typed = len(want["node_clv"]), want["typed"][0]
    inner = {int(c): "N%d" % k for k, c in enumerate(want["node_clv"])}

    def name_of(k, c):
        child = int(want["node_children"][k, c])
        return inner[child] if child in inner else tree.tip_label(child)

    # ---- one row per branch
    rows = [l.split("\t") for l in open(prefix + ".substitutions.tsv").read().splitlines()]
    pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
    assert rows[0] == (["node", "child", "name", "length", "expected_total"] + ["%s>%s" % ("ACGT"[i], "ACGT"[j]) for i, j in pairs] +
                       ["dwell_%s" % ch for ch in "ACGT"] + ["change_probability_sum"])
    assert len(rows) == 1 + 2 * n
    for r, (k, c) in zip(rows[1:], ((k, c) for k in range(n) for c in range(2))):
        assert r[:3] == ["N%d" % k, str(c), name_of(k, c)]
        assert abs(float(r[3]) - want["lengths"][k, c]) <= 1e-10
        e = [typed[k, c, i, j] for i, j in pairs]
        assert [float(x) for x in r[5:17]] == e   # (%.17g: the bits)
        assert abs(float(r[4]) - sum(e)) <= 1e-12 * sum(e)
        assert [float(x) for x in r[17:21]] == [typed[k, c, i, i] for i in range(4)]
        changed = float((weights * want["change"][k, c]).sum())
        assert abs(float(r[21]) - changed) <= 1e-12 * max(changed, 1.0)
    # identity D in the file: the dwell times of a branch add up to its length times the number of columns
    for r in rows[1:]:
        assert abs(sum(float(x) for x in r[17:21]) - float(r[3]) * len(pattern_of)) <= 1e-8 * len(pattern_of)

    # ---- one row per (branch, column) at or above the threshold, in branch and column order
    got = [l.split("\t") for l in open(prefix + ".mutations.tsv").read().splitlines()]
    assert got[0] == ["node", "child", "name", "partition", "column", "from", "to", "probability", "expected_count"]
    expect = []
    for k in range(n):
        for c in range(2):
            for col, pat in enumerate(pattern_of):
                if want["top_prob"][k, c, pat] >= min_prob:
                    code = int(want["top_pair"][k, c, pat])
                    expect.append(["N%d" % k, str(c), name_of(k, c), "0", str(col + 1), "ACGT"[code // 4], "ACGT"[code % 4],
                                   want["top_prob"][k, c, pat], want["count"][k, c, pat]])
    assert len(expect) > 0 and len(got) == 1 + len(expect)
    for r, e in zip(got[1:], expect):
        assert r[:7] == e[:7] and float(r[7]) == e[7] and float(r[8]) == e[8]
        assert r[5] != r[6]

    # ---- the names of the rows are the names of the tree
    newick = open(prefix + ".substitutions.tree").read()
    assert rd.Tree.from_newick(newick).tip_count() == 10
    names = [r[2] for r in rows[1:]]
    assert len(set(names)) == 2 * n and set(inner.values()) - set(names) == {"N0"}   # the root hangs under no branch
    for name in names:
        if name in inner.values():
            assert ")%s:" % name in newick, name
        else:
            assert re.search(r"[(,]%s:" % re.escape(name), newick), name
    tree.root_by(rl)
    assert newick == tree.newick_ancestral(want["node_clv"])
    line = next(l for l in out.stdout.splitlines() if l.startswith("Substitutions at root"))
    assert abs(float(line.split("lnL ")[1].split(",")[0]) - want["lnl"]) <= 1e-6 * abs(want["lnl"])

    # ---- the same run without the option: every shared output byte for byte, nothing new
    out2 = _run(common + ["--prefix", plain])
    assert out2.returncode == 0, out2.stdout + out2.stderr
    made = sorted(f[len("subst"):] for f in os.listdir(tmp_path) if f.startswith("subst"))
    shared = sorted(f[len("plain"):] for f in os.listdir(tmp_path) if f.startswith("plain"))
    assert sorted(set(made) - set(shared)) == NEW
    for ext in shared:
        if ext != ".ckp":   # (the checkpoint's header holds the prefix)
            assert open(plain + ext, "rb").read() == open(prefix + ext, "rb").read(), ext
    assert [l for l in out.stdout.splitlines() if not l.startswith("Substitutions at root")] == out2.stdout.splitlines()

    # ---- refused where --gradient is
    refused = _run(["--msa", MSA, "--tree", TREE, "--silent", "--prefix", str(tmp_path / "no"), "--exhaustive",
                    "--site-shards", "2", "--substitutions"])
    assert refused.returncode != 0
    assert "--substitutions" in refused.stdout + refused.stderr and "--site-shards" in refused.stdout + refused.stderr
    assert not os.path.exists(str(tmp_path / "no") + ".substitutions.tsv")
