"""CPU: the committed fixtures under tests/golden/ cover the regimes in which the GPU tests would otherwise rest on the
oracle alone, so that the pinning of the oracle to the reference binaries cannot shrink unnoticed:

  * every model kind the GPU tests build has a fixture;
  * a FLASH-BS run at B >= 1024 (cfg5's width);
  * beam misses (-1 in the recorded path) with N > 1 — "later tasks restart from Pi" — at least three, on at least two kinds;
  * a model where ties alone decide the path at K > 1024;
  * every fixture's hashes are those of the model tests/modelgen.py rebuilds from its spec (golden_model asserts it).

(tests/test_oracle_golden.py compares the oracle with every recorded run.)"""
import os

from conftest import GOLDEN_DIR, golden_model, load_goldens

KINDS = ("data_script", "ties_all", "ties_semi", "wideA", "wideB", "wideAB", "rotor", "rotor_tied_column", "circulant_ties",
         "unreachable")
TIE_KINDS = ("ties_all", "ties_semi", "circulant_ties")
GOLDENS = load_goldens(include_big=True)


def runs(algo=None):
    return [(g, r) for g in GOLDENS for r in g["runs"] if algo is None or r["algo"] == algo]


def test_every_kind_has_a_fixture():
    have = {g["spec"]["kind"] for g in GOLDENS}
    assert set(KINDS) <= have, sorted(set(KINDS) - have)
    # the rotor with and without noise: chains that merge slowly, and never
    assert {bool(g["spec"]["noise"]) for g in GOLDENS if g["spec"]["kind"] == "rotor"} == {False, True}
    # every kind but the tied rotor column (a FLASH-BS model) has a whole-sequence full-state run
    for kind in KINDS:
        assert any(r["algo"] == "flash" and r["N"] == 1 for g, r in runs() if g["spec"]["kind"] == kind), kind
        assert any(r["algo"] == "flashbs" for g, r in runs() if g["spec"]["kind"] == kind), kind


def test_a_beam_as_wide_as_cfg5s():
    wide = [(g["name"], r["N"]) for g, r in runs("flashbs") if r["B"] >= 1024]
    assert wide and {n for _, n in wide} >= {1, 8}, wide


def test_beam_misses_with_more_than_one_task():
    miss = [(g["name"], g["spec"]["kind"], r["N"], r["B"]) for g, r in runs("flashbs") if r["N"] > 1 and -1 in r["path"]]
    assert len(miss) >= 3 and len({kind for _, kind, _, _ in miss}) >= 2, miss
    assert ("wideB_K600_T60", "wideB", 4, 2) in miss
    # a miss leaves found entries beside the -1s: the tasks to the right of it went on
    for g, r in runs("flashbs"):
        if -1 in r["path"]:
            assert any(s >= 0 for s in r["path"]), (g["name"], r["N"], r["B"])


def test_ties_beyond_1024_states():
    assert any(g["spec"]["kind"] in TIE_KINDS and g["spec"]["K"] > 1024 for g in GOLDENS)


def test_backtracks_longer_than_one_lane_walks():
    """T = 300 on the rotors: a chain of more than 128 steps, where the 64-lane walk starts"""
    assert all(g["spec"]["T"] > 129 for g in GOLDENS if g["spec"]["kind"] == "rotor")


def test_fixture_hashes_match_the_rebuilt_models():
    for g in GOLDENS:
        A, B, Pi, ob = golden_model(g)          # asserts the hashes and the observation list
        assert A.shape == (g["spec"]["K"],) * 2 and B.shape == (g["spec"]["K"], g["spec"]["M"]) and len(ob) == g["spec"]["T"], g["name"]


def test_fixtures_are_small_and_hold_data_only():
    keys = {"name", "spec", "ob", "sha", "runs", "provenance"}
    run_keys = {"algo", "N", "B", "step", "path", "memory", "score", "ref_time_s"}
    for g in GOLDENS:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, g["name"] + ".json")) < 16 * 1024, g["name"]
        assert set(g) == keys and all(set(r) <= run_keys for r in g["runs"]), g["name"]
