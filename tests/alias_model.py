"""The alias-table sweep of DESIGN 11e in numpy float32: what k_alias_classify and k_alias_sweep compute, written from the
specification (one pass over the `over` and `under` lists from the back, carrying one float), not from the host function's two
piles.  tests/test_light_rebuild_cpu.py pins it to hostlib.build_alias_table bit for bit."""
import numpy as np

F = np.float32
TABLE_DTYPE = np.dtype([("prob", "<f4"), ("failId", "<i4")])


def sweep(values, drop_subtraction_at=None):
    """values float32[n] -> (table TABLE_DTYPE[n], sum float32).  drop_subtraction_at = k leaves step k's `r - (1 - p)` out (a
    planted mistake for the distribution check)."""
    values = np.ascontiguousarray(values, dtype=F)
    n = len(values)
    table = np.zeros(n, TABLE_DTYPE)
    with np.errstate(all="ignore"):
        s = F(0)
        for x in values:  # strictly sequential, index order
            s = F(s + x)
        scale = F(F(n) / s) if n else F(0)
        val = (values * scale).astype(F)
        over = [i for i in range(n) if val[i] > F(1)]
        under = [i for i in range(n) if not val[i] > F(1)]
        o, u = len(over), len(under)  # unread entries: [0, o), [0, u)
        big = pend = None             # (index, prob)
        step = 0
        while True:
            if big is None:
                if o == 0:
                    break
                o -= 1
                big = (over[o], val[over[o]])
            if pend is None:
                if u == 0:
                    break
                u -= 1
                small = (under[u], val[under[u]])
            else:
                small, pend = pend, None
            table[small[0]] = (small[1], big[0])
            r = big[1] if step == drop_subtraction_at else F(big[1] - F(F(1) - small[1]))
            step += 1
            big = (big[0], r)
            if not r > F(1):
                pend, big = big, None
        for e in (big, pend):
            if e is not None:
                table[e[0]] = (e[1], e[0])
        for i in over[:o] + under[:u]:
            table[i] = (val[i], i)
    return table, s


def encoded_distribution(table):
    """float64: the probability with which sampling `table` returns each entry — (prob_i + sum over j with failId_j = i of
    (1 - prob_j)) / n."""
    n = len(table)
    prob = table["prob"].astype(np.float64)
    p = prob.copy()
    np.add.at(p, table["failId"], 1.0 - prob)
    return p / n


def power_sets():
    """{name: float32 values}: the sets the CPU and GPU tests share (the deformed scenes' light powers are added by the tests)."""
    rng = np.random.default_rng(20)
    return {
        "one": np.array([3.0], F),
        "seven equal": np.full(7, 0.25, F),
        "two": np.array([1.0, 3.0], F),
        "65 uniform": rng.uniform(0, 1, 65).astype(F),
        "500 small, one huge": np.concatenate([np.full(500, 1e-3, F), np.array([1e4], F)]),
        "777 over nine decades": (10.0 ** rng.uniform(-6, 3, 777)).astype(F),
        "1000 uniform": rng.uniform(0, 1, 1000).astype(F),
        "4097 exponential": rng.exponential(1.0, 4097).astype(F),
        "leading zeros": np.concatenate([np.zeros(5, F), rng.uniform(0.1, 2, 70).astype(F)]),
    }
