"""The alias-table sweep (tests/alias_model.py) against the host's two-pile construction, and a float64 check that a
table encodes the distribution it was built from."""
import numpy as np
import pytest

import alias_model
import light_deform
from helpers import assert_bit_equal


@pytest.fixture(scope="module")
def power_sets():
    from radish_pt_amd import scenes

    sets = dict(alias_model.power_sets())
    for g in ((4, 8), (16, 32)):
        sd = scenes.teapots(segments=24, bands=18, emissive_grid=g)
        for step in (0, 1):
            sets[f"teapots {g} step {step}"] = light_deform.light_powers(sd, light_deform.deformed_vertices(sd, step))
    return sets


def test_model_equals_host_table(power_sets):
    from radish_pt_amd import hostlib

    for name, values in power_sets.items():
        ht, hs = hostlib.build_alias_table(values)
        mt, ms = alias_model.sweep(values)
        assert_bit_equal(np.array([ms], np.float32), np.array([hs], np.float32), f"{name}: sum")
        assert np.array_equal(mt["failId"], ht["failId"]), f"{name}: failId differs at {np.flatnonzero(mt['failId'] != ht['failId'])[:5]}"
        assert_bit_equal(mt["prob"], ht["prob"], f"{name}: prob")


def test_model_all_zero_and_nan():
    """sum == 0: every val is NaN, nothing is above the mean, the table is {NaN, i}."""
    from radish_pt_amd import hostlib

    z = np.zeros(65, np.float32)
    ht, _ = hostlib.build_alias_table(z)
    mt, _ = alias_model.sweep(z)
    assert np.isnan(ht["prob"]).all() and np.isnan(mt["prob"]).all()
    assert np.array_equal(mt["failId"], np.arange(65)) and np.array_equal(ht["failId"], np.arange(65))
    v = np.array([1.0, np.nan, 2.0, 0.5], np.float32)  # a NaN among the values poisons the sum: the same places on both sides
    ht, _ = hostlib.build_alias_table(v)
    mt, _ = alias_model.sweep(v)
    assert np.array_equal(np.isnan(mt["prob"]), np.isnan(ht["prob"])) and np.array_equal(mt["failId"], ht["failId"])


def _margin(n):
    """First-order bound on |encoded_i - values_i / sum| for a table built in binary32 from non-negative values, u = 2^-24.
    With q_i = values_i / sum exact and m_i = n * encoded_i:
      * the sequential sum carries n - 1 roundings, the division and the product one each: val_i = n q_i (1 + b_i), |b_i| <= (n + 1) u,
        so |val_i - n q_i| <= n (n + 1) u, and summed over i the same bound holds (sum of q_i = 1);
      * a step turns r into r - (1 - p) + e with |e| <= u (|1 - p| + |r'|) <= u (1 + r) <= u (n + 1); there are at most n - 1 steps, so
        all e together stay below (n - 1)(n + 1) u;
      * an entry finalised by a step has m_i = val_i + its own e's.  An entry of the tail names itself and keeps 1 - prob_i too; the
        sum of m_i is n exactly, so those leftovers sum to -(sum of (val_i - n q_i)) - (sum of e), and they all have one sign (the
        tail is what is left of ONE list), so each is at most n (n + 1) u + (n - 1)(n + 1) u.
    Together |m_i - n q_i| <= 4 n (n + 1) u."""
    return 4.0 * (n + 1) * 2.0 ** -24


def _deviation(table, values):
    v = values.astype(np.float64)
    return np.abs(alias_model.encoded_distribution(table) - v / v.sum()).max()


def test_table_encodes_its_distribution(power_sets):
    from radish_pt_amd import hostlib

    for name, values in power_sets.items():
        for what, table in (("host", hostlib.build_alias_table(values)[0]), ("model", alias_model.sweep(values)[0])):
            dev = _deviation(table, values)
            assert dev <= _margin(len(values)), f"{name} ({what}): {dev:.3e} > {_margin(len(values)):.3e}"


def test_distribution_check_catches_planted_mistakes(power_sets):
    values = power_sets["65 uniform"]
    table, _ = alias_model.sweep(values)
    m = _margin(len(values))
    assert _deviation(table, values) <= m
    # two entries' failIds swapped: the two with the most different probs among those that fail to different entries
    donors = np.flatnonzero(table["failId"] != np.arange(len(table)))
    a = donors[np.argmin(table["prob"][donors])]
    others = donors[table["failId"][donors] != table["failId"][a]]
    b = others[np.argmax(table["prob"][others])]
    swapped = table.copy()
    swapped["failId"][[a, b]] = table["failId"][[b, a]]
    assert _deviation(swapped, values) > m
    # one step's subtraction dropped
    dropped, _ = alias_model.sweep(values, drop_subtraction_at=0)
    assert _deviation(dropped, values) > m
