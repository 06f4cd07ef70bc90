"""CPU: the two certificates of the O2 -> CO2 conversion's ladder (pyset_order_check in csrc/sim_core.h, through
tests/native/set_order_mixed_host.cpp) against real CPython sets, in the style of tests/test_set_order_cert.py. Keys are float 3-tuples
like the sinks and arrive group by group. Every group has a TRUE order (the cKDTree's, in the simulator) and a provisional one (the
sink indices'). Rung 0 walks the provisional stream and flags the groups whose order can matter (X). Rung 1 certifies the mixed
stream -- X's groups in true order, the others provisional. Wherever it does, list(set) of the mixed stream under EVERY tried order
of the groups outside X must equal the set built in the true order throughout."""
import ctypes
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "native", "set_order_mixed_host.cpp")
    so = os.path.join(ROOT, "tests", "native", "libsetordermixedhost.so")
    deps = [src] + [os.path.join(ROOT, "octa_autosegmentation_amd", "csrc", f) for f in ("sim_core.h", "sim_host.h", "gpow.h", "glibc_pow_tables.h", "glibc_trig.h", "glibc_trig_tables.h")]
    if not os.path.exists(so) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    l = ctypes.CDLL(so)
    l.octa_setcert_flag_groups.restype = ctypes.c_int
    l.octa_setcert_flag_groups.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    l.octa_setcert_second.restype = ctypes.c_int
    l.octa_setcert_second.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    return l


def _arrays(groups):
    keys = [k for g in groups for k in g]
    h = (ctypes.c_ulonglong * max(1, len(keys)))(*[hash(k) & MASK64 for k in keys])
    gi = (ctypes.c_int * max(1, len(keys)))(*[i for i, g in enumerate(groups) for _ in g])
    return h, gi, len(keys)


def flag(lib, groups):
    """rung 0 on a stream -> (number of violations, X as a list of flags per group)"""
    h, gi, n = _arrays(groups)
    buf = ctypes.create_string_buffer(max(1, len(groups)))
    v = lib.octa_setcert_flag_groups(h, gi, n, buf, len(groups))
    return v, [buf.raw[g] != 0 for g in range(len(groups))]


def second(lib, groups, x):
    h, gi, n = _arrays(groups)
    return bool(lib.octa_setcert_second(h, gi, n, bytes(1 if f else 0 for f in x) or b"\0", len(groups)))


def _py_order(groups):
    s = set()
    for g in groups:
        for k in g:
            s.add(k)
    return list(s)


def _orders_outside_x(true, x, rng, n_random):
    """X's groups in true order; the others in every joint order when there are few, else the provisional one and n_random random ones."""
    free = [i for i, g in enumerate(true) if not x[i] and len(g) > 1]
    total = 1
    for i in free:
        for f in range(2, len(true[i]) + 1):
            total *= f
        if total > 720:
            break
    if total <= 720:
        for perm in itertools.product(*[itertools.permutations(true[i]) for i in free]):
            order = [list(g) for g in true]
            for i, p in zip(free, perm):
                order[i] = list(p)
            yield order
        return
    for _ in range(n_random):
        yield [list(g) if x[i] else rng.sample(g, len(g)) for i, g in enumerate(true)]


def _key(rng, clustered):
    """A random sink-like tuple; `clustered`: only tuples whose hash has a few low-bit patterns (crowded probe sequences)."""
    while True:
        t = (rng.random(), rng.random(), rng.random() * 0.1)
        if not clustered or (hash(t) & 31) < 3:
            return t


def _stream(rng, n_groups, max_size, clustered):
    """Groups of mostly one or two keys, some up to max_size, each in its true order."""
    sizes = [1 if rng.random() < 0.85 else rng.randint(2, max_size) for _ in range(n_groups)]
    return [[_key(rng, clustered) for _ in range(n)] for n in sizes]


def _mixed(true, prov, x):
    return [list(t) if f else list(p) for t, p, f in zip(true, prov, x)]


@pytest.mark.parametrize("n_groups,max_size,clustered", [(3, 3, True), (6, 4, True), (12, 6, False), (12, 6, True),
                                                         (40, 5, False), (40, 3, True), (120, 2, False), (300, 2, False)])
def test_second_certificate_fixes_the_table_for_every_order_outside_x(lib, n_groups, max_size, clustered):
    """Across small tables (8, 32 slots) and several resizes. The shares are bounded both ways: some streams certify as they stand, some
    only with X in true order, and the second certificate refuses at most half of the 150 (in the simulator it refuses 9 of 3 821 flagged
    conversions; these mostly-single-key streams hardly ever make it refuse: the refusals' lower bound is asserted on the crowded family
    and on the constructed stream below)."""
    rng = random.Random(2000 * n_groups + 10 * max_size + clustered)
    rung0 = partial = refused = 0
    for _ in range(150):
        true = _stream(rng, n_groups, max_size, clustered)
        prov = [sorted(g) for g in true]                       # the provisional order: by the key itself, as the sink index is
        v, x = flag(lib, prov)
        assert (v == 0) == (not any(x)), "every violation names a group"
        assert all(len(true[i]) > 1 for i, f in enumerate(x) if f), "only a group of several keys can be flagged"
        ref = _py_order(true)
        if v == 0:
            rung0 += 1
            assert second(lib, prov, x), "nothing flagged: the second certificate is the first"
        elif not second(lib, _mixed(true, prov, x), x):
            refused += 1
            continue
        else:
            partial += 1
        for order in _orders_outside_x(true, x, rng, 40):
            assert _py_order(order) == ref, "certified, but an order inside a group outside X changes the set's order"
    print(f"{n_groups} groups: certified as they stand {rung0}, with X in true order {partial}, refused {refused}")
    assert rung0 >= 5 and partial >= 5
    assert refused <= 75           # the second certificate passes for most flagged streams (the simulator's: 9 refusals in 3 821)


def _crowded_key(rng, bits, patterns):
    """A sink-like tuple whose hash falls on one of `patterns` home slots of the table with 2 ** bits slots."""
    while True:
        t = (rng.random(), rng.random(), rng.random() * 0.1)
        if (hash(t) & ((1 << bits) - 1)) < patterns:
            return t


@pytest.mark.parametrize("n_groups,bits,patterns", [(2, 3, 2), (5, 5, 3), (6, 5, 4), (16, 7, 6), (20, 7, 10), (24, 7, 16)])
def test_crowded_multi_key_groups_make_the_second_certificate_refuse(lib, n_groups, bits, patterns):
    """Streams in which putting X into true order really moves keys of other groups: EVERY group has two or three keys, and all keys
    are at home on a few slots of the table the stream ends in (4 - 6 keys: 8 slots, or 32 from the fifth key on; 10 - 18 keys: 32 slots;
    32 - 72 keys: 128 slots), so groups
    share their probe paths within a generation and across the resizes. The second certificate must refuse some of these streams
    (at least 5 of 300, and at most half), and some of the refused ones must really depend on an order outside X; where it passes,
    every tried order outside X gives the table of the true order, and some of the passing streams do have a multi-key group outside X."""
    rng = random.Random(100 * n_groups + patterns)
    partial = refused = dependent = with_free = 0
    for _ in range(300):
        true = [[_crowded_key(rng, bits, patterns) for _ in range(rng.randint(2, 3))] for _ in range(n_groups)]
        prov = [sorted(g) for g in true]
        v, x = flag(lib, prov)
        ref = _py_order(true)
        if v and not second(lib, _mixed(true, prov, x), x):
            refused += 1
            if any(_py_order(order) != ref for order in _orders_outside_x(true, x, rng, 40)):
                dependent += 1
            continue
        partial += 1 if v else 0
        with_free += 0 if all(x) else 1
        for order in _orders_outside_x(true, x, rng, 40):
            assert _py_order(order) == ref, "certified, but an order inside a group outside X changes the set's order"
    print(f"{n_groups} groups on {patterns} of {1 << bits} slots: with X in true order {partial}, of them with a group outside X {with_free}, "
          f"refused {refused}, of them order-dependent {dependent}")
    assert 5 <= refused <= 150 and dependent >= 1
    assert partial >= 5 and with_free >= 5


def test_everything_flagged_is_always_certified(lib):
    """All groups in X: the whole stream stands in its true order, nothing is provisional."""
    rng = random.Random(13)
    for _ in range(200):
        true = _stream(rng, rng.randint(1, 60), 5, True)
        assert second(lib, true, [True] * len(true))


def test_two_keys_of_a_group_on_one_home_slot_flag_that_group(lib):
    """The flagging is not vacuous: two keys of one group on the same home slot of an 8-slot table put that group (and only it) in X,
    and the table really depends on their order in some of these streams. With that group in true order the stream certifies."""
    rng = random.Random(7)
    dependent = 0
    for _ in range(200):
        first = [_key(rng, False)]
        while hash(first[0]) & 7 == 0:
            first = [_key(rng, False)]
        a = _key(rng, False)
        while hash(a) & 7 != 0:
            a = _key(rng, False)
        b = _key(rng, False)
        while hash(b) & 7 != 0:
            b = _key(rng, False)
        true = [first, [a, b]]
        prov = [first, [b, a]]
        v, x = flag(lib, prov)
        assert v > 0 and x == [False, True]
        assert second(lib, _mixed(true, prov, x), x)
        if _py_order(true) != _py_order(prov):
            dependent += 1
    assert dependent > 0


def _second_probe(k):
    """second slot of k's probe sequence in an 8-slot table (no linear probes there: i + 9 > mask)"""
    h = hash(k) & MASK64
    return (5 * (h & 7) + 1 + (h >> 5)) & 7


def _key_where(rng, cond):
    while True:
        k = _key(rng, False)
        if cond(k):
            return k


def test_second_certificate_refuses_where_x_in_true_order_moves_another_group(lib):
    """Rung 0 judges the groups outside X on the table of the PROVISIONAL order; putting X into its true order moves X's keys. 8-slot table:
    group 0 = (a, b), both at home on slot h, second slots sa != sb. Provisional (b, a) holds h and sa, the true order (a, b) holds h and sb.
    Group 1 = (c, d): c at home on sb with second slot t, d at home on t. On the provisional table c takes sb and d takes t, no key passes a
    sibling: only group 0 is flagged. With group 0 in true order b holds sb, c moves on to t, and d now passes c: the second certificate
    must refuse, and the table does depend on the order of (c, d) in some of these streams."""
    rng = random.Random(99)
    dependent = 0
    for _ in range(100):
        a = _key(rng, False)
        h, sa = hash(a) & 7, _second_probe(a)
        if sa == h:
            continue
        b = _key_where(rng, lambda k: hash(k) & 7 == h and _second_probe(k) not in (h, sa))
        sb = _second_probe(b)
        c = _key_where(rng, lambda k: hash(k) & 7 == sb and _second_probe(k) not in (h, sa, sb))
        t = _second_probe(c)
        d = _key_where(rng, lambda k: hash(k) & 7 == t)
        true, prov = [[a, b], [c, d]], [[b, a], [c, d]]
        v, x = flag(lib, prov)
        assert v > 0 and x == [True, False]
        assert not second(lib, _mixed(true, prov, x), x)
        assert second(lib, true, [True, True])
        if _py_order([[a, b], [d, c]]) != _py_order(true):
            dependent += 1
    print(f"order-dependent outside X: {dependent}")
    assert dependent > 0


def test_a_straddled_resize_flags_the_straddling_group(lib):
    """Six keys on distinct home slots: a group that straddles the resize (the 5th distinct key of the 8-slot table) is flagged although
    nothing collides, and is certified once it stands in true order."""
    rng = random.Random(3)
    for _ in range(50):
        keys, used = [], set()
        while len(keys) < 6:
            k = _key(rng, False)
            h8, h32 = hash(k) & 7, hash(k) & 31
            if h8 in {u & 7 for u in used} or h32 in used:
                continue
            used.add(h32)
            keys.append(k)
        assert flag(lib, [keys[:5], keys[5:]]) == (0, [False, False])
        v, x = flag(lib, [keys[:4], keys[4:]])
        assert v > 0 and x == [False, True]
        assert second(lib, [keys[:4], keys[4:]], x)
        assert not second(lib, [keys[:4], keys[4:]], [False, False])
