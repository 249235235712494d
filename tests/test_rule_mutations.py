"""Mutation testing of the product's rule headers: which CPU test pins which clause of rg_policy.h, rg_policy_grad.h, rg_action_mask.h, rg_path.h, rg_route.h,
rg_objects.h, rg_monsters.h, rg_novelty.h and the scout part of rg_episode.h?

The kernels and their CPU twins compile the same headers, so the GPU tests ("kernel equals twin, bit for bit") are blind to a wrong rule.  tests/rule_mutants.py
lists one textual misreading per clause; each is built for the host twins alone in a temporary directory and the header's *_host.py files run against it.  The
result must equal the committed map (tests/golden/rule_pins.json, regenerated with profiles/rule_pin_map.txt by tools/rule_pin_map.py), every mutant of class
`rule` must be noticed by a named test, and every `equivalent` one must carry the reason why no output can change (and be noticed by none).

CPU only; no mutant is ever compiled for the device.  All 104 mutants in one pool took 316 s here (8 cores, 4 workers of 4 compilers each: 16 processes at the
most), about 12 s a mutant -- more than five minutes, so the map is checked in one case per header.  Measured per case, the unmutated build included:
rg_objects.h 165 s (the unmutated build runs that header's play tests, the mutants die in the hand-answered cases before them), rg_policy.h 103 s,
rg_monsters.h 63 s, rg_action_mask.h 58 s, rg_policy_grad.h 54 s, the other four 25 to 38 s each; 9.5 minutes in all."""
import json
import os
import re

import pytest

from rule_mutants import EQUIVALENT, MUTANTS, RULE, TESTS, kill_matrix, occurrences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = os.path.join(ROOT, "tests", "golden", "rule_pins.json")


@pytest.fixture(scope="module", autouse=True)
def built():
    """The product's libraries and objects, as every host test builds them; the probe itself only reads the checkout."""
    import __graft_entry__ as g
    g.build()


def test_every_old_text_stands_exactly_once_in_its_header():
    occ = occurrences()
    assert all(v == 1 for v in occ.values()), {k: v for k, v in occ.items() if v != 1}
    names = [m["name"] for m in MUTANTS]
    assert len(set(names)) == len(names) and 80 <= len(names) <= 120
    assert {m["header"] for m in MUTANTS} == set(TESTS)
    for m in MUTANTS:
        assert m["old"] != m["new"] and m["clause"] and m["cls"] in (RULE, EQUIVALENT), m["name"]
        assert (m["cls"] == EQUIVALENT) == bool(m["reason"]), "%s: an equivalent mutant carries its reason, a rule mutant none" % m["name"]
        assert all(os.path.exists(os.path.join(ROOT, "tests", f if isinstance(f, str) else f[0])) for f in TESTS[m["header"]])


@pytest.mark.parametrize("header", sorted(TESTS))
def test_pin_map_matches_the_committed_one(header):
    res = kill_matrix([header])
    assert res.pop("") is None, "the unmutated build fails a test of %s" % (TESTS[header],)
    want = {m["name"]: v for m in MUTANTS if m["header"] == header for v in [json.load(open(PINS))[m["name"]]]}
    assert res == want, {k: (res.get(k), want.get(k)) for k in set(res) | set(want) if res.get(k) != want.get(k)}
    for m in MUTANTS:
        if m["header"] == header:
            if m["cls"] == RULE:
                assert res[m["name"]] is not None, "%s misreads '%s' and no test of %s notices" % (m["name"], m["clause"], TESTS[header])
            else:
                assert res[m["name"]] is None, "%s is classed equivalent, but %s notices it" % (m["name"], res[m["name"]])


def test_the_published_map_names_every_mutant():
    pins = json.load(open(PINS))
    assert set(pins) == {m["name"] for m in MUTANTS}
    text = open(os.path.join(ROOT, "profiles", "rule_pin_map.txt")).read()
    for m in MUTANTS:
        assert re.search(r"^%s\s+%s\s" % (re.escape(m["name"]), m["cls"]), text, re.M), "%s is missing from profiles/rule_pin_map.txt" % m["name"]
        if pins[m["name"]]:
            assert "<- " + pins[m["name"]] in text
            f, t = pins[m["name"]].split("::")
            assert re.search(r"^def %s\(" % re.escape(t), open(os.path.join(ROOT, "tests", f)).read(), re.M), "%s names a test that does not exist" % m["name"]
