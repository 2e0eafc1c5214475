"""Which code every k runs: the engine's choice of the minimizer length m (mic_engine.hip: decide_layout), the t-mer length of
mod-sampling (mic_device.h: s_tlen) and the launcher's routing (mic_kernels.hip: mic_launch_query, mic_query_kernel_name) restated in
plain Python, and the list of (k, m) that tests/test_k_sweep_gpu.py runs against the oracle.  The list must reach every combination
of the four keys the query kernels branch on that ANY k and any MIC_MINIMIZER_LEN reach; nothing here needs a GPU.

    w = k - m + 1     m-mers per k-mer (a super-k-mer entry holds windows of at most 16)
    t = s_tlen(k, m)  t = m - j w with the largest j that keeps t >= 7
    W = k - t + 1     t-mers per k-mer: the window of the sliding minimum

  key               values                                        where it branches
  t                 <= 12 | 13 .. 16 | > 16                       sampled_positions: s_torder24 / s_torder with its high term /
                                                                  kmer_from_dwords and 64-bit t-mers; s_sampled in the build
  W                 < 16 | 16 | > 16, (W - 16) % 4 == 0 | other   sliding_min3 / sliding_min_rows: one row pair, one round, two
  W against w       W == w | W == 2 w | other                     i mod w: nothing / one conditional subtraction / (d * rcp) >> 10
  kernel family     query_kernel_s one-strand; query_kernel_r one-strand and two-strand, each with k and m from the table
                    ("generic") or as constants (k = 27, 31, 32 with m = 20); query_kernel_m (the minimizer layout)
"""
import itertools

import pytest

DIRECT, MINIMIZER, SUPER, SUPER2 = 1, 2, 3, 4
K_MIN, K_MAX = 12, 32            # below 12 no m >= 8 leaves a window of 5: every layout falls back to the direct one
CONSTANT_K = (27, 31, 32)        # instantiations with k and m = 20 as constants (query_kernel_m: 27 and 31 only)


# ------------------------------------------------------------------ the restatement

def decide_layout(k, layout, env_m=None):
    """(layout, m) the engine arrives at for a requested layout and a MIC_MINIMIZER_LEN of env_m (None: not set); m = 0 on the
    direct layout, as mic_db_get_info reports it"""
    m = 20 if env_m is None else env_m
    m = min(m, k - 4, 31)
    if layout == MINIMIZER and (m < 8 or k - m + 1 > 64):
        layout = DIRECT
    if layout in (SUPER, SUPER2):
        m = max(m, k - 15)
        if m < 8 or m > 31 or k - m + 1 < 2:
            layout = DIRECT
    return layout, (0 if layout == DIRECT else m)


def s_tlen(k, m):
    w, t = k - m + 1, m
    while t - w >= 7:
        t -= w
    return t


def geometry(k, m):
    w, t = k - m + 1, s_tlen(k, m)
    return w, t, k - t + 1


def run_ok(k, m):
    """the one-strand per-run kernel reverse-complements a region of 2k - m nucleotides inside three words, realigned by one funnel shift"""
    return 32 < 2 * k - m <= 48


def kernel_name(k, m, layout, parted=False, key_bytes=8):
    """the instantiation mic_db_kernel_name reports (MIC_S_GENERIC and MIC_S_PER_KMER not set, no bucket-range shard)"""
    b = ("false", "true")
    if layout in (SUPER, SUPER2):
        fw = layout == SUPER2
        kk, mm = (k, m) if m == 20 and k in CONSTANT_K else (0, 0)
        if fw or run_ok(k, m):
            return f"query_kernel_r<{kk}, {mm}, {b[fw]}, {b[parted]}>"
        return f"query_kernel_s<{kk}, {mm}, {b[parted]}, false>"      # a slot-range part filters in the `sharded` instantiation
    if layout == MINIMIZER:
        kk, mm = (k, m) if m == 20 and k in (27, 31) else (0, 0)
        return f"query_kernel_m<{kk}, {mm}>"
    return f"query_kernel<{b[key_bytes == 8]}>"


def family(k, m, layout):
    if layout == MINIMIZER:
        return "query_kernel_m"
    if layout == SUPER and not run_ok(k, m):
        return "query_kernel_s one-strand"
    const = m == 20 and k in CONSTANT_K
    return f"query_kernel_r {'two' if layout == SUPER2 else 'one'}-strand {'constant' if const else 'generic'}"


def branch_keys(k, m, layout):
    """(t, W, W against w, kernel family); the minimizer layout's kernel takes plain minimizers: no t-mers, no window of them"""
    if layout == MINIMIZER:
        return (None, None, None, family(k, m, layout))
    w, t, W = geometry(k, m)
    return ("t <= 12" if t <= 12 else "t 13..16" if t <= 16 else "t > 16",
            "W < 16" if W < 16 else "W = 16" if W == 16 else "W > 16, one round" if (W - 16) % 4 == 0 else "W > 16, two rounds",
            "W = w" if W == w else "W = 2w" if W == 2 * w else "W other",
            family(k, m, layout))


def front_half(k, m):
    """the front half's road in words"""
    w, t, W = geometry(k, m)
    if (k, m) == (31, 20):
        return "sampled_positions3 (per-run kernel), sliding_min_rows one round bm 3 (per-k-mer kernel)"
    smin = ("sliding_min3" if W < 16 else "sliding_min_rows, one row pair" if W == 16 else
            f"sliding_min_rows, one round, bank mask {(1 << ((W - 16) >> 2)) - 1}" if (W - 16) % 4 == 0 else "sliding_min_rows, two rounds")
    mod = "no modulo" if W == w else "one subtraction" if W == 2 * w else "(d * rcp) >> 10"
    order = "s_torder24" if t <= 12 else "s_torder, high term" if t <= 16 else "kmer_from_dwords, 64-bit t-mers"
    return f"{order}; {smin}; {mod}"


# ------------------------------------------------------------------ the list

DEFAULT_K = list(range(K_MIN, K_MAX + 1))
# (k, MIC_MINIMIZER_LEN): what no k reaches with the default m.  Each is the only pair of the list for at least one combination
# (test_every_other_m_is_needed names it).  Among them: t = 16 (the run-time shift of revcomp_bits32) at W = 16 and below it, t > 16,
# W = w (no modulo) on every family, W = 24 and 20 through the generic sliding_min_rows, w = 16 (the widest entry) and
# k = 27 / 31 / 32 on the instantiations without constants.  Where several m reach a combination the longer one stands here: with
# 4^8 .. 4^11 minimizer values a table of 300 000 k-mers has most of its minimizers crowded, and the reads would be answered by
# the side table and the dense fallback, not by the front half under test.
OTHER_M = [(31, 16), (32, 17), (27, 17), (24, 12),
           (27, 12), (26, 19), (31, 24), (27, 21), (30, 16), (19, 13), (29, 22), (32, 23), (31, 23), (25, 18), (24, 16), (26, 22)]
SWEEP = [(k, decide_layout(k, SUPER)[1]) for k in DEFAULT_K] + OTHER_M          # (k, m) as the table reports it


def reachable():
    """every (k, m) a super-k-mer table can have: any k the layouts take, any value of MIC_MINIMIZER_LEN"""
    pairs = set()
    for k, env_m in itertools.product(range(1, K_MAX + 1), [None] + list(range(-1, 70))):
        layout, m = decide_layout(k, SUPER, env_m)
        if layout == SUPER:
            pairs.add((k, m))
    return sorted(pairs)


def combinations_of(pairs, default_k=DEFAULT_K):
    """branch-key combinations a list of (k, m) reaches on the two super-k-mer layouts, and the minimizer layout's for the default m"""
    got = {branch_keys(k, m, layout) for k, m in pairs for layout in (SUPER, SUPER2)}
    return got | {branch_keys(k, decide_layout(k, MINIMIZER)[1], MINIMIZER) for k in default_k}


# ------------------------------------------------------------------ the tests

def test_default_m_and_the_table_of_the_design_notes():
    """the engine's m, t, W and kernel for every k with the default m: the table in DESIGN.md 3.4.1"""
    assert [decide_layout(k, SUPER) for k in (8, 11)] == [(DIRECT, 0)] * 2 and decide_layout(11, MINIMIZER) == (DIRECT, 0)
    assert decide_layout(K_MIN, SUPER) == (SUPER, 8) and decide_layout(K_MIN, MINIMIZER) == (MINIMIZER, 8)
    want = {24: (20, 10, 15, "query_kernel_s<0, 0, false, false>"), 25: (20, 8, 18, "query_kernel_s<0, 0, false, false>"),
            26: (20, 13, 14, "query_kernel_s<0, 0, false, false>"), 27: (20, 12, 16, "query_kernel_r<27, 20, false, false>"),
            28: (20, 11, 18, "query_kernel_r<0, 0, false, false>"), 29: (20, 10, 20, "query_kernel_r<0, 0, false, false>"),
            30: (20, 9, 22, "query_kernel_r<0, 0, false, false>"), 31: (20, 8, 24, "query_kernel_r<31, 20, false, false>"),
            32: (20, 7, 26, "query_kernel_r<32, 20, false, false>")}
    for k, (m, t, W, name) in want.items():
        assert decide_layout(k, SUPER) == (SUPER, m) and geometry(k, m)[1:] == (t, W) and kernel_name(k, m, SUPER) == name, k
    for k in range(K_MIN, 24):
        m = k - 4
        assert decide_layout(k, SUPER2) == (SUPER2, m) and geometry(k, m)[0] == 5 and geometry(k, m)[1] <= 12
        assert kernel_name(k, m, SUPER) == "query_kernel_s<0, 0, false, false>" and kernel_name(k, m, SUPER2) == "query_kernel_r<0, 0, true, false>"
    # only k = 26 has t > 12 and only k = 29 and 31 the one-round window with the default m
    assert [k for k in DEFAULT_K if geometry(k, decide_layout(k, SUPER)[1])[1] > 12] == [26]
    assert [k for k in DEFAULT_K if branch_keys(k, decide_layout(k, SUPER)[1], SUPER)[1] == "W > 16, one round"] == [29, 31]
    # slot-range parts: the per-k-mer kernel filters in its sharded instantiation, the per-run kernels in their own
    assert kernel_name(26, 20, SUPER, parted=True) == "query_kernel_s<0, 0, true, false>"
    assert kernel_name(29, 20, SUPER, parted=True) == "query_kernel_r<0, 0, false, true>"
    assert kernel_name(29, 20, SUPER2, parted=True) == kernel_name(24, 20, SUPER2, parted=True) == "query_kernel_r<0, 0, true, true>"
    assert kernel_name(31, 20, MINIMIZER) == "query_kernel_m<31, 20>" and kernel_name(32, 20, MINIMIZER) == "query_kernel_m<0, 0>"


def test_the_other_m_are_what_the_arithmetic_says():
    geo = {(k, m): geometry(k, m) for k, m in OTHER_M}
    assert geo[(31, 16)] == (16, 16, 16) and geo[(32, 17)] == (16, 17, 16) and geo[(27, 17)] == (11, 17, 11) and geo[(24, 12)] == (13, 12, 13)
    assert geo[(30, 16)] == (15, 16, 15) and geo[(27, 12)] == (16, 12, 16) and geo[(31, 24)] == (8, 8, 24) and geo[(26, 22)] == (5, 7, 20)
    for k, m in OTHER_M:
        assert decide_layout(k, SUPER, m) == (SUPER, m) and decide_layout(k, SUPER2, m) == (SUPER2, m)      # the engine keeps the value as given
        assert kernel_name(k, m, SUPER2) == "query_kernel_r<0, 0, true, false>"
        assert kernel_name(k, m, SUPER) == ("query_kernel_r<0, 0, false, false>" if run_ok(k, m) else "query_kernel_s<0, 0, false, false>")
    assert run_ok(24, 12) and not run_ok(24, 20) and not run_ok(24, 16) and not run_ok(19, 13)


def test_the_sweep_reaches_every_reachable_combination():
    pairs = reachable()
    assert min(k for k, m in pairs) == K_MIN and all(8 <= m <= 28 and 5 <= k - m + 1 <= 16 for k, m in pairs)
    want = combinations_of(pairs)
    assert len(want) == 46 + 1                   # super-k-mer layouts + minimizer layout (a change of the rules shows here first)
    assert {c[0] for c in want} == {None, "t <= 12", "t 13..16", "t > 16"} and len({c[3] for c in want}) == 6
    assert set(SWEEP) <= set(pairs) and len(set(SWEEP)) == len(SWEEP)
    got = combinations_of(SWEEP)
    assert got == want, sorted(want - got, key=str)


def test_every_k_has_its_case():
    assert [k for k, m in SWEEP[:len(DEFAULT_K)]] == list(range(12, 33))
    assert all(decide_layout(k, SUPER) == (SUPER, m) for k, m in SWEEP[:len(DEFAULT_K)])


@pytest.mark.parametrize("pair", OTHER_M)
def test_every_other_m_is_needed(pair):
    """without the pair a combination is uncovered (so the list carries no case that repeats another one's road)"""
    rest = [p for p in SWEEP if p != pair]
    lost = combinations_of(SWEEP) - combinations_of(rest)
    assert lost, pair


def test_division_by_w_as_multiply_and_shift():
    """sampled_positions: d < 32, w <= 16: (d * rcp) >> 10 = d / w exactly, rcp = ceil(1024 / w)"""
    for w in range(2, 17):
        rcp = (1024 + w - 1) // w
        for d in range(32):
            assert (d * rcp) >> 10 == d // w, (d, w)
    # it is the bound on d that makes it exact: the first miss for the w in use lies beyond 32
    first_miss = min(d for w in range(2, 17) for d in range(32, 4096) if (d * ((1024 + w - 1) // w)) >> 10 != d // w)
    assert first_miss > 32 + 31


def test_unreachable_arms_of_the_bank_mask_switch():
    """sliding_min_rows switches on bm = 2^((W - 16) / 4) - 1 when W > 16 and (W - 16) % 4 == 0.  t >= 7 and k <= 32 bound W = k - t + 1
    by 26, so W is 20 or 24 there and bm 1 or 3: the arms `case 7` (W = 28) and `default` (bm 15, W = 32) are dead code today.  They
    stay in the kernel; this is the place that says so."""
    pairs = reachable()
    assert min(geometry(k, m)[1] for k, m in pairs) == 7 and max(geometry(k, m)[2] for k, m in pairs) == 26
    one_round = {geometry(k, m)[2] for k, m in pairs if geometry(k, m)[2] > 16 and (geometry(k, m)[2] - 16) % 4 == 0}
    assert one_round == {20, 24}
    assert {(1 << ((W - 16) >> 2)) - 1 for W in one_round} == {1, 3}
    assert {geometry(k, m)[2] for k, m in SWEEP} >= one_round          # and the sweep runs both live arms
