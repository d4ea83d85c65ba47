"""The overlap-add advance table (tests/ola_advance_signals.py): what can be checked about it without a GPU.

Every figure of the table is a literal, checked here against the oracle's record of a row's run (oracle_py.Oracle
.increments and its output): the set of advances, the histogram of leads (P mod (N + 4)) mod 4, the ring wraps, the
non-finite samples and, for the overrun rows, the dropped slices and the leads they pile up at.  The regime claims --
which branch of pv_kernels.hip chain_slice_tail / chain_finish_slice a row is there for -- are stated on those literals.
The engine's planner (engine.plan_simulate) has to give the same per-call counts and the same increments."""
import numpy as np
import pytest

from audiomod_amd import engine as E
from oracle import oracle_py as O
from tests import ola_advance_signals as S

NONFINITE_CAP = 0.15   # of a row's oracle output
PEAK_MIN = 0.01
F = S.FIGURES


def test_the_table_has_a_figure_for_every_defined_row_and_no_other():
    assert sorted(F) == sorted(S.DEFINED)
    assert [r.name for r in S.ROWS if r.kind == S.UNDEFINED] == ["rob512_h513", "p512_+4_h407"]
    assert [r.name for r in S.ROWS if r.kind == S.ENGINE_REFUSES] == ["p512_-24_h4"]
    assert len(S.SERVED) == 50


@pytest.mark.parametrize("name", S.DEFINED)
def test_every_literal_is_what_the_oracle_gives(name):
    assert S.figures(name) == F[name]
    run = S.oracle(name)
    assert run.info["slices"] == F[name][0] == sum(run.slices_per_call)
    # the cap on non-finite samples, and audio in what is left: from the oracle alone
    fin = np.isfinite(run.y)
    assert np.count_nonzero(~fin) == F[name][4] <= NONFINITE_CAP * run.y.size
    assert float(np.abs(run.y[fin]).max()) > PEAK_MIN
    assert run.y.shape[1] >= S.BY_NAME[name].frames


@pytest.mark.parametrize("name", S.DEFINED)
def test_the_planner_gives_the_oracles_counts_and_increments(name):
    row = S.BY_NAME[name]
    run = S.oracle(name)
    calls = S.call_list(name, len(run.counts))
    if row.kind == S.ENGINE_REFUSES:
        with pytest.raises(E.PvError):
            E.plan_simulate(calls, channels=row.channels, **row.cfg)
        return
    avail, shift, _, info = E.plan_simulate(calls, channels=row.channels, **row.cfg)
    assert [int(a) for a in avail] == list(run.counts)
    assert np.array_equal(shift, run.shift)
    assert info["slices"] == F[name][0]
    assert (info["hop_in"], info["resample"]) == (row.cfg["hopsize"], run.info["resample"])


def test_robotic_rows_advance_by_the_hop():
    for r in S.ROBOTIC_ROWS + S.OVERRUN_ROWS:
        assert F[r.name][1] == (r.cfg["hopsize"],), r.name
        assert not S.oracle(r.name).info["resample"]


def test_plain_rows_advance_as_the_increment_recurrence_gives():
    want = {"p512_+4_h2": (2, 3), "p512_-24_h8": (2,), "s512_0.3_h8_core1": (2, 3), "s512_0.3_h8_core0": (2, 3),
            "p1024_+7_h340": (509, 510), "p2048_+7_h1020": (1528, 1529), "p2048_+4_h1621": (2042, 2043),
            "p1024_+12_h511": (1022,), "p1024_+12_h512": (1024,), "p512_+4_h406": (511, 512),
            "s512_1.5_h341_core2": (511, 512), "s512_1.5_h340_core0": (510,), "g512_-7_h300": (200, 201),
            "s2048_1.5_h1360": (2040,), "p512_-24_h4": (1,)}
    assert {n: F[n][1] for n in want} == want
    assert sorted(want) == sorted(r.name for r in S.PLAIN_ROWS + S.REFUSED_ROWS)
    # resampling down, up 1:4, and none
    assert S.oracle("p512_+4_h2").info["res_num"] > S.oracle("p512_+4_h2").info["res_den"]
    i = S.oracle("p512_-24_h8").info
    assert (i["res_num"], i["res_den"]) == (1, 4)
    assert not S.oracle("s512_0.3_h8_core1").info["resample"]
    assert S.oracle("p1024_+12_h511").info["int_ratio"] == 1


# ---- the regimes, on the literals
def _leads(name):
    return F[name][2]


def _adv(name):
    return F[name][1]


def test_all_four_leads_occur_at_the_smallest_advances():
    for n in ("rob512_h1", "rob512_h3", "rob512_h5", "rob256_h1", "p512_+4_h2", "p1024_+7_h340"):
        assert min(_leads(n)) > 0, n
    # an even advance keeps to even leads, a multiple of four to lead 0: the engine's own hops in the fixed-advance modes
    assert _leads("rob512_h2")[1::2] == (0, 0) and _leads("rob512_h64")[1:] == (0, 0, 0)


def test_scalar_masks_and_the_in_place_test_both_sides():
    """chain_slice_tail: the first two pieces (samples up to 512 - lead) get scalar zero-masks, piece j >= 2 the test
    256 j - lead < advance.  At fft 512 (two pieces, and the tail quad of a shifted frame as piece 2) it is met for an
    advance above 512 - lead only; at fft 1024 ... 4096 by every advance above 509."""
    for n in ("rob512_h507", "rob512_h508", "rob512_h509"):   # piece 2 never reaches in: 512 - 3 >= advance
        assert max(_adv(n)) <= 509
    for n in ("rob512_h511", "p512_+4_h406", "s512_1.5_h341_core2"):   # 512 - lead < advance for leads 2, 3 (and 1 at 512)
        assert max(_adv(n)) >= 511 and _leads(n)[2] > 0 and _leads(n)[3] > 0
    assert _adv("rob512_h512") == (512,) and _leads("rob512_h512")[1:] == (0, 0, 0)   # 512 - 0 < 512 is false: the edge
    # fft 1024: either side of piece 2 (256 * 2 - lead < advance) with every lead, and of piece 3 (768 - lead)
    assert _adv("rob1024_h509") == (509,) and _adv("rob1024_h512") == (512,) and _adv("rob1024_h515") == (515,)
    assert _adv("p1024_+7_h340") == (509, 510)
    assert _adv("rob1024_h765") == (765,) and _adv("rob1024_h769") == (769,)
    for n in ("rob1024_h509", "rob1024_h515", "rob1024_h765", "rob1024_h769", "rob1024_h1021", "rob1024_h1023"):
        assert min(_leads(n)) > 0, n
    # the last piece at each size, one and three samples short of N and N itself
    for n, N in (("rob1024_h1021", 1024), ("rob1024_h1023", 1024), ("rob2048_h2045", 2048), ("rob2048_h2047", 2048),
                 ("rob4096_h4093", 4096), ("p2048_+4_h1621", 2048)):
        assert N - 6 <= max(_adv(n)) < N and min(_leads(n)) > 0, n


def test_denominator_prefetch_both_sides_of_64_and_128_quads():
    """fin_quads = (advance + lead + 3) >> 2 clamps the address of a lane's denominators; lanes 0 ... 63 prefetch
    quads 0 ... 63 and 64 ... 127, later pieces load late"""
    def quads(n):
        return {(a + lead + 3) >> 2 for a in _adv(n) for lead in range(4) if _leads(n)[lead]}
    assert quads("rob1024_h253") == {64}
    assert quads("rob512_h255") == {64, 65} and quads("rob512_h256") == {64} and quads("rob512_h257") == {65}
    assert quads("rob512_h63") == {16, 17} and quads("rob512_h65") == {17}
    assert quads("rob512_h507") == {127, 128} and quads("rob512_h509") == {128}
    assert quads("rob512_h511") == {128, 129} and quads("rob1024_h515") == {129, 130}
    assert quads("rob512_h1") == {1} and quads("rob512_h5") == {2}


def test_generic_sizes_take_the_prefix_and_the_loop():
    """chain_finish_slice (fft 256 and 8192): 4 x 64 samples in registers, a loop from sample 256 on, and advances
    below 64 where most lanes idle"""
    (a,) = _adv("rob256_h1")
    assert a < 64                                  # one lane of the prefix's first group, nothing else
    (a,) = _adv("rob256_h255")
    assert 3 * 64 < a < 4 * 64                     # all four groups of the prefix, the last one short of a lane; no loop
    (a,) = _adv("rob256_h256")
    assert a == 4 * 64                             # the prefix exactly full: the loop's first index 256 + lane is out
    (a,) = _adv("rob8192_h8189")
    assert a > 256 and (a - 256) % 64 != 0         # the loop, many rounds, the last one partial
    assert S.BY_NAME["rob8192_h8189"].channels == 1
    for n in ("rob256_h1", "rob256_h255", "rob8192_h8189"):   # the generic kernel indexes sample by sample: every lead
        assert min(_leads(n)) > 0, n


def test_an_advance_of_n_gives_non_finite_samples_and_nothing_else_does():
    for n in S.DEFINED:
        N = S.fft_of(n)
        assert (F[n][4] > 0) == (max(_adv(n)) == N), n
    assert {n: F[n][4] for n in S.DEFINED if F[n][4]} == {
        "rob512_h512": 30, "rob1024_h1024": 22, "rob2048_h2048": 28, "rob256_h256": 30, "p1024_+12_h512": 3968,
        "p512_+4_h406": 2046, "s512_1.5_h341_core2": 34}


def test_every_row_wraps_the_ring():
    for n in S.DEFINED:
        assert F[n][3] >= 2, n


def test_overrun_rows_drop_slices_at_every_lead():
    a, b = (F[n] for n in S.OVERRUN)
    assert a[5:] == (486, (0, 162, 0, 324)) and b[5:] == (643, (214, 214, 215, 0))
    both = tuple(x + y for x, y in zip(a[6], b[6]))
    assert all(both[lead] >= 1 for lead in (1, 2, 3))
    for n in S.OVERRUN:
        run = S.oracle(n)
        assert max(run.counts) >= run.info["outbuf_capacity"] - 2 * run.info["fftsize"]   # the ring really fills up


def test_undefined_rows_are_undefined_in_the_oracle_and_refused_by_the_planner():
    for r in S.ROWS:
        if r.kind != S.UNDEFINED:
            continue
        with pytest.raises(O.OracleUndefined):
            S.oracle(r.name)
        with pytest.raises(E.PvError, match="undefined behaviour in the reference") as e:
            E.plan_simulate([S.BLOCK] * 40, channels=r.channels, **r.cfg)
        assert "unsupported configuration" in str(e.value)
        with pytest.raises(E.PvError, match="undefined behaviour in the reference"):   # decided before any device call
            E.Batch(3, r.frames, channels=r.channels, **r.cfg)
        with pytest.raises(E.PvError, match="undefined behaviour in the reference"):
            E.mbatch_layout([(r.frames, r.cfg.get("semitones", 0.0), 1.0)], channels=r.channels,
                            **{k: v for k, v in r.cfg.items() if k != "semitones"})


REASON = "hop too small for this ratio: the smallest shift increment a slice can take"


def test_a_hop_whose_smallest_increment_rounds_to_zero_is_refused_at_creation_with_the_reason():
    """fft 512, -24 st, hop 4: hop x ratio = 1 and the increment clamp's lower end lrint(1 / 2) is 0.  The reference runs
    it (every advance is 1: FIGURES); the engine sizes its frame rings by that lower end and refuses, in every form, at
    creation and before any device call, saying why.  One hop up (lrint(2 / 2) = 1) is served: the row p512_-24_h8."""
    (row,) = S.REFUSED_ROWS
    assert F[row.name][1] == (1,)
    cfg = row.cfg
    makes = [lambda: E.plan_simulate([480], channels=2, **cfg),
             lambda: E.PhaseVocoder(48000, 2, 1.0, cfg["semitones"], E.NORMAL_SHIFT, E.PHASE_LOCKED, 512, cfg["hopsize"]),
             lambda: E.Batch(3, row.frames, channels=2, **cfg),
             lambda: E.StreamPool(3, channels=2, **cfg),
             lambda: E.HostIO(3, row.frames, channels=2, **cfg),
             lambda: E.mbatch_layout([(row.frames, cfg["semitones"], 1.0)], channels=2, mode=cfg["mode"], fftsize=512,
                                     hopsize=cfg["hopsize"])]
    for make in makes:
        with pytest.raises(E.PvError) as e:
            make()
        assert REASON in str(e.value) and "below 1" in str(e.value), str(e.value)
    info = E.plan_simulate([480], channels=2, **S.config("p512_-24_h8"))[3]
    assert info["hop_in"] == 8
    assert E.lib().pv_last_error() in (b"", None)   # the text does not outlive the call that set it


def test_tile_path_limit_flips_between_hop_7_and_hop_6():
    """Core::init: the tile path holds at most 128 frames per tile -- (tile span + N) / smallest advance + 3, the span
    260 samples without resampling -- so ROBOTIC at fft 512 is on it down to hop 7 and beyond it from hop 6"""
    assert (260 + 512) // 7 + 3 == 113 <= 128 < (260 + 512) // 6 + 3 == 131
