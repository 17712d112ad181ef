"""The alignment kernels (seed.hip: the seed kernel; rows.hip: the 32- and
64-lane row kernels; finish.hip: first_finish_kernel, the later-seed rounds;
extend.hip: extend_kernel; align.hip: the order of their passes) on the
hand-built cases of tests/align_cases.py, against the C oracle bit for bit.

tests/test_align_cases_host.py shows on the CPU which edge of the spec each
case lands on (the band's two edges, the 32-lane window, the X-drop
comparison, DMAX, transcript ends, MAX_HSP, the e-value cut in each direction,
the bit-score print rule) and that a second implementation agrees with the
oracle there. Here one engine run per parameter set goes through every HSP of
both directed searches, then the tables, edges and distances (full_check); a
difference names the case of the first differing transcript. The counters
prove that the path a setting is about really ran.
"""
import itertools

import pytest

import align_cases as ac
from oracle.parity import INT_FIELDS, full_check

pytestmark = pytest.mark.gpu


def _run(cor, **kw):
    from rna_clique_amd.engine import Engine
    eng = Engine(device=0, **kw)
    for s in cor.samples:
        eng.add_sample(s.name, s.seq, s.tx_offsets, s.gene, s.iso)
    eng.run()
    return eng


def _rows(arr, base_q, base_s):
    """{query transcript: [record]} of one directed search, in output order."""
    out = {}
    for h in arr:
        out.setdefault(int(h["q_tx"]) - base_q, []).append(
            (int(h["s_tx"]) - base_s, *(int(h[f]) for f in INT_FIELDS)))
    return out


def check(eng, cor, **params):
    """Every HSP of every directed search against the oracle, named by case;
    then tables, edges, ideal nodes, sums and distances. Returns the number of
    oracle HSPs."""
    from oracle.align import OracleDB
    db = OracleDB(cor.samples)
    n = 0
    for q, s in itertools.permutations(range(len(cor.samples)), 2):
        ora = db.align(q, s, params.get("word_size", 28), params.get("xdrop_half", 108),
                       params.get("evalue", 1e-99), eng.symmetric, eng.dust)
        n += len(ora)
        want = _rows(ora, db.tx_base[q], db.tx_base[s])
        got = _rows(eng.hsps(q, s), 0, 0)
        for t in sorted(set(want) | set(got)):
            assert got.get(t, []) == want.get(t, []), \
                (f"search {q}->{s}, {cor.case_of(t)}: GPU {got.get(t, [])} vs oracle {want.get(t, [])} "
                 f"(s_tx, {', '.join(INT_FIELDS)})")
    msgs, _ = full_check(eng, cor.samples, check_hsps=False, **params)
    assert not msgs, "\n".join(msgs[:10])
    tm = eng.timings()
    assert tm["defer_length"] == 0 and tm["defer_gaveup"] == 0
    return n


# ------------------------------------------------------------------ the short corpus

SETTINGS = {
    "default": ({}, {}),
    "share0": ({"RC_SHARE": "0"}, {}),
    "symmetric": ({}, {"symmetric": True, "dust": False}),
    "dust_off": ({}, {"dust": False}),
    "win4": ({"RC_WIN_WORDS": "4"}, {}),
    "win9": ({"RC_WIN_WORDS": "9"}, {}),
    "resume": ({"RC_RESUME": "1"}, {}),
    "later0": ({"RC_LATER": "0"}, {}),
    "later_rows32": ({"RC_LATER_ROWS": "32"}, {}),
    "later_cap3": ({"RC_LATER_CAP": "3"}, {}),
}
# a loose e-value lets the short HSPs through (MAX_HSP blocks, seeds at the
# word size): the settings about later seeds are run with it as well. The
# ambiguous-base kernels (a corpus with N) take the settings that pick a kernel.
RUNS = ([(k, False, 1e-99) for k in SETTINGS] +
        [(k, True, 1e-99) for k in ("default", "share0", "win4", "resume", "later_rows32")] +
        [(k, False, 10.0) for k in ("default", "later0", "later_rows32", "later_cap3")])


KNOBS = ("RC_SHARE", "RC_WIN_WORDS", "RC_RESUME", "RC_LATER", "RC_LATER_ROWS", "RC_LATER_CAP")


def _setenv(monkeypatch, env):
    """The knobs of this file: the ones in env set, the others at their defaults."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in KNOBS
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("setting,amb,evalue", RUNS, ids=[f"{k}-{'amb' if a else 'acgt'}-{e:g}" for k, a, e in RUNS])
def test_short_corpus(native, monkeypatch, setting, amb, evalue):
    """Band edges, window spans, X-drop boundaries, transcript ends, early
    stops, seeds, MAX_HSP and the e-value cut, four placements each, under
    every path the knobs select. The counters: the corpus holds live spans
    past 32 (the 64-lane pass), band-stopped and MAX_HSP pairs (later seeds)."""
    env, kw = SETTINGS[setting]
    _setenv(monkeypatch, env)
    cor = ac.short_corpus(amb)
    with _run(cor, evalue=evalue, **kw) as eng:
        assert check(eng, cor, evalue=evalue) > 100
        tm = eng.timings()
    # (the 64-lane lists and the later-seed rounds belong to shared searches:
    # not symmetric mode, not RC_SHARE=0)
    shared = env.get("RC_SHARE") != "0" and not kw.get("symmetric")
    if shared:
        assert tm["ext_wide"] > 0
    if shared and env.get("RC_LATER") != "0":
        assert tm["later_seeds"] > 0
    elif shared:
        assert tm["later_seeds"] == 0 and tm["defer_outside"] > 0
    else:   # every search with a seed outside its first box goes to extend_kernel
        assert tm["later_seeds"] == 0 and tm["ext_deferred"] > 0
    assert (tm["later_whole"] > 0) == ("RC_LATER_CAP" in env)


def test_early_stop_step_count(native, monkeypatch):
    """The row kernels stop an extension as soon as no live diagonal's bound
    (its score if every remaining base matched) exceeds best -- the oracle has
    no such test, and the result is the same either way, so only the step
    counter shows it. On pairs that end at a transcript end right after a
    mismatch and k matching bases (k = 2: the bound EQUALS best) every
    extension takes exactly the steps of the trace's kernel_steps, none when
    the first slide reaches a transcript end."""
    from extend_trace import codes, search_pair
    _setenv(monkeypatch, {})
    cor = ac.step_count_corpus()
    calls = steps = 0
    for t in range(len(cor.entries)):
        a, b = (s.seq[int(s.tx_offsets[t]):int(s.tx_offsets[t + 1])].tobytes() for s in cor.samples)
        kept, boxes = search_pair(codes(a), codes(b))
        assert len(boxes) == 1 and max(boxes[0].left.span, boxes[0].right.span) < 16
        calls += 2
        steps += boxes[0].left.kernel_steps + boxes[0].right.kernel_steps
    assert steps == sum(1 for c, p in cor.entries if c.cls == "early_stop")
    with _run(cor, dust=False) as eng:
        check(eng, cor)
        tm = eng.timings()
    print(f"ext_calls {tm['ext_calls']:.0f} (trace {calls}), ext_steps {tm['ext_steps']:.0f} (trace {steps})")
    assert (tm["ext_calls"], tm["ext_steps"]) == (calls, steps)


# ------------------------------------------------------------------ the long corpus


@pytest.mark.parametrize("env", [{}, {"RC_SHARE": "0"}, {"RC_LATER": "0"}], ids=["default", "share0", "later0"])
def test_long_corpus(native, monkeypatch, env):
    """Transcripts of 16 to 54 kb (windowed staging): an extension that stops
    at DMAX = 4096 differences on either strand, its twin that ends one
    difference short of it, and identical transcripts on both sides of the
    bit score's switch to %5.3le."""
    _setenv(monkeypatch, env)
    cor = ac.long_corpus()
    with _run(cor) as eng:
        assert check(eng, cor) >= 2 * len(cor.entries)
        bits = sorted(int(h["bits10"]) for h in eng.hsps(0, 1) if cor.entries[int(h["q_tx"])][0].cls == "bits")
    assert bits == [999040, 999970, 1000000, 1001000]


# ------------------------------------------------------------------ options


@pytest.mark.parametrize("W", [16, 17, 29, 64])
def test_word_size(native, monkeypatch, W):
    """The seed kernel's stride W - 15 other than 13: exact runs of W - 1, W
    and W + 1 at every phase of the stride, on both strands, cut by an N, at
    transcript ends (a loose e-value lets HSPs of W bases through), and a
    simulated corpus with indels and minus-strand transcripts."""
    from rna_clique_amd.simulate import simulate
    _setenv(monkeypatch, {})
    cor = ac.seed_corpus(W)
    with _run(cor, word_size=W, evalue=10.0) as eng:
        assert check(eng, cor, word_size=W, evalue=10.0) > 2 * (W - 15)
        # the run whose only aligned word of the lower sample is DUST-masked
        assert W < 23 or eng.timings()["reverse_seeds"] > 0
    samples, _ = simulate(3, 60, seed=16 + W, indel_rate=0.004, p_revcomp=0.5)
    sim = ac.Corpus(samples, [])
    with _run(sim, word_size=W) as eng:
        msgs, summary = full_check(eng, samples, word_size=W)
        assert not msgs, "\n".join(msgs[:10])
        assert summary["hsps"] > 0


@pytest.mark.parametrize("X", [0, 1, 20, 1000])
def test_xdrop_half(native, monkeypatch, X):
    _setenv(monkeypatch, {})
    cor = ac.short_corpus(False)
    with _run(cor, xdrop_half=X) as eng:
        assert check(eng, cor, xdrop_half=X) > 100


@pytest.mark.parametrize("evalue", [1e-5, 10.0])
def test_evalue(native, monkeypatch, evalue):
    _setenv(monkeypatch, {})
    cor = ac.short_corpus(True)
    with _run(cor, evalue=evalue) as eng:
        assert check(eng, cor, evalue=evalue) > 100


def test_option_refusals(native):
    from rna_clique_amd._native import NativeError, RC_E_ARG
    from rna_clique_amd.engine import Engine
    for kw in ({"word_size": 15}, {"word_size": 65}, {"xdrop_half": -1}):
        with pytest.raises(NativeError) as ei:
            Engine(device=0, **kw)
        assert ei.value.code == RC_E_ARG, kw
    for kw in ({"word_size": 16}, {"word_size": 64}, {"xdrop_half": 0}):
        Engine(device=0, **kw).close()
