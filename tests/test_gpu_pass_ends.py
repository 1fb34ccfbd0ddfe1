"""GPU: the ends of a pass — final_argmax / final_argmax_batch, last_column / last_column_csr, backtrack / backtrack_flat
(backtrack_walk) with flat_resolve, and the walk inside beam_end_backtrack — on models built to make them work hard, with
the regime asserted.

The models (tests/modelgen.py):
  rotor            every state has one successor; without noise no two back-track chains ever merge, so every chunk of the
                   64-lane walk that did not start from the truth fails its check and the retry branch runs up to 63
                   times in one walk.  fv_stats.bt_restarts must equal the retries tests/backtrack_model.py counts on the
                   oracle's arg table.
  circulant_ties   every finite score of a step is the same float: each back-pointer is the lowest live predecessor and
                   each end pick the lowest live state, with the tied candidates up to 2000 states apart — in different
                   lanes, waves, 256-blocks (the trips of last_column's gathers) and 1024-blocks (the trips of
                   final_argmax's loop).  The facts are asserted from the oracle's tables before the GPU is judged.
  rotor_tied_column  a rotor with one column that is tied at almost every time: a tagged cell that only a wrongly guessed
                   chain of the FLASH-BS walk runs through must not make the decode rebuild its layouts.

Bar: equality.  Paths equal, scores equal as uint32, return codes equal; expected values from the oracle only."""
import numpy as np
import pytest

import backtrack_model as btm
import modelgen
import oracle
from flash_viterbi_amd import decoder
from test_gpu_row_codes import band_model, raw_full
from test_pass_end_models import ROTOR_T, check_circulant, circulant_model, observations, rotor_formula, rotor_model

pytestmark = pytest.mark.gpu

D = decoder
SPLITS = (1, 2, 4, 7)
DENSE_KERNELS = (D.KERNEL_F64_STREAM, D.KERNEL_F32_REFINE, D.KERNEL_F16_REFINE, D.KERNEL_Q16_REFINE, D.KERNEL_SPARSE_Q16,
                 D.KERNEL_U16_REFINE)
EAGER_LAYOUTS = 1 << 19          # FV_OPT_DEBUG: heap layouts and tie fix-up always, no lazy first walk


def bits(x):
    return int(np.float32(x).view(np.uint32))


def whole_pass(om, ob):
    """(path, score bits, retries of the 64-lane walk) of one forward pass over the sequence with the lowest-index end
    pick and the plain back-track, from the oracle's tables"""
    T = len(ob)
    row, args = om.full_forward(ob, 0, T - 1, -1)
    end = int(np.argmax(row))                                  # (first of the maxima)
    table = args.tolist()
    chain = btm.serial_walk(table, 0, T - 1, end)
    walked, restarts = btm.chunk_walk(table, 0, T - 1, end)
    assert walked == chain
    return chain + [end], bits(row[end]), restarts


def got_of(res):
    path, score, rc = res
    return path.tolist(), bits(score), rc


@pytest.fixture(scope="module")
def ctx():
    made = {}

    def get(key, setter):
        if key not in made:
            fv = decoder.FlashViterbi(0)
            setter(fv)
            made[key] = fv
        fv = made[key]
        fv.set_option(D.OPT_DEBUG, 0)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_AUTO)
        fv.set_option(D.OPT_FLAT_GENERATIONS, D.FLAT_AUTO)
        return fv
    yield get
    for fv in made.values():
        fv.close()


def dense_ctx(ctx, name, A, Bm, Pi):
    return ctx(("dense", name), lambda fv: fv.set_model(A, Bm, Pi))


def sparse_ctx(ctx, name, A, Bm, Pi):
    return ctx(("sparse", name), lambda fv: fv.set_model_sparse(*decoder.dense_to_csr(A), Bm, Pi))


# ---------------------------------------------------------------- 1. rotor, full-state

@pytest.mark.parametrize("T", ROTOR_T)
@pytest.mark.parametrize("noise", [0, 0.02, 0.2])
@pytest.mark.parametrize("K", [61, 257])
def test_rotor_full_state(ctx, K, noise, T):
    A, Bm, Pi, om = rotor_model(K, noise)
    ob = observations(7, T, 1000 + T)
    fv = dense_ctx(ctx, ("rotor", K, noise), A, Bm, Pi)
    fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
    path, score, restarts = whole_pass(om, ob)
    print(f"rotor K={K} noise={noise} T={T}: the whole pass's walk retries {restarts} times")
    # the regime: a chain of 127 steps is walked by one lane; longer ones retry (no noise: as often as the arithmetic says)
    assert (restarts == 0) if T - 1 < btm.BT_MIN_PARALLEL else (restarts > 0)
    if noise == 0:
        assert restarts == rotor_formula(T - 1)
    got = got_of(fv.decode_full(ob, 1, D.MODE_SINGLE_PASS))
    st = fv.stats()
    assert got == (path, score, 0)
    assert st["bt_restarts"] == restarts
    for n in SPLITS:
        opath, oscore, _, orc = om.full_decode(ob, n)
        got = got_of(fv.decode_full(ob, n, D.MODE_REFERENCE))
        st = fv.stats()
        assert got == (opath.tolist(), bits(oscore), orc) and orc == 0, n
        # (the whole-sequence pass is one of its back-tracks: at least that pass's retries, more from the long right-hand ones)
        assert st["bt_restarts"] >= restarts and (st["bt_restarts"] > 0) == (T - 1 >= btm.BT_MIN_PARALLEL), (n, st["bt_restarts"])
    vpath, vscore, vrc = om.vanilla_decode(ob)
    assert got_of(fv.decode_vanilla(ob)) == (vpath.tolist(), bits(vscore), vrc)
    # (the baselines round in another order: with noise a near-tie may fall the other way and the chain merge elsewhere)
    assert fv.stats()["bt_restarts"] == restarts or noise != 0
    for step in (0, 200):
        cpath, cscore, crc = om.checkpoint_decode(ob, step)
        assert got_of(fv.decode_checkpoint(ob, step)) == (cpath.tolist(), bits(cscore), crc), step
        assert fv.stats()["bt_restarts"] == restarts or noise != 0, step


def test_rotor_on_a_sparse_set_model(ctx):
    """last_column_csr and init_rows_csr at the ends of the right-hand passes, the same walk behind them"""
    K, noise, T = 61, 0.02, 2050
    A, Bm, Pi, om = rotor_model(K, noise)
    ob = observations(7, T, 1000 + T)
    fv = sparse_ctx(ctx, ("rotor", K, noise), A, Bm, Pi)
    path, score, restarts = whole_pass(om, ob)
    assert restarts > 0
    for kernel in (D.KERNEL_AUTO, D.KERNEL_CSR_F64):
        fv.set_option(D.OPT_KERNEL, kernel)
        assert got_of(fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)) == (path, score, 0)
        assert fv.stats()["bt_restarts"] == restarts
        for n in SPLITS:
            opath, oscore, _, orc = om.full_decode(ob, n)
            assert got_of(fv.decode_full(ob, n, D.MODE_REFERENCE)) == (opath.tolist(), bits(oscore), orc), (kernel, n)
            st = fv.stats()
            assert st["bt_restarts"] >= restarts and st["column_steps"] > 0, (kernel, n)


# ---------------------------------------------------------------- 2. flat route

@pytest.mark.parametrize("noise", [0, 0.02])
@pytest.mark.parametrize("n", [2, 4])
def test_rotor_flat_generations(ctx, n, noise):
    """backtrack_flat walks every right-hand pass of the plan in one launch (the long ones by 64 lanes), flat_resolve commits
    them; with a poisoned snapshot entry the resolver stops and the generations are run again one by one."""
    K, T = 61, 2050
    A, Bm, Pi, om = rotor_model(K, noise)
    ob = observations(7, T, 1000 + T)
    fv = dense_ctx(ctx, ("rotor", K, noise), A, Bm, Pi)
    fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
    opath, oscore, _, orc = om.full_decode(ob, n)
    want = (opath.tolist(), bits(oscore), orc)
    stats = {}
    for flat in (D.FLAT_OFF, D.FLAT_ON):
        fv.set_option(D.OPT_FLAT_GENERATIONS, flat)
        assert got_of(fv.decode_full(ob, n, D.MODE_REFERENCE)) == want, flat
        stats[flat] = fv.stats()
    off, on = stats[D.FLAT_OFF], stats[D.FLAT_ON]
    print(f"rotor K={K} noise={noise} n_split={n}: flat passes {on['flat_passes']}, retries flat {on['bt_restarts']} / by generation {off['bt_restarts']}")
    assert off["flat_passes"] == 0 and on["flat_passes"] > 0 and on["flat_first_miss"] == -1
    assert on["bt_restarts"] > 0 and off["bt_restarts"] > 0
    # every chain was committed, so both forms walked the same chains from the same ends
    assert on["bt_restarts"] == off["bt_restarts"]
    # a long pass of the second generation loses the state it is conditioned on: the resolver falls back
    long_pass = next(p for p in decoder.plan_flat(T, n) if p["generation"] == 2 and p["R"] - p["L"] >= btm.BT_MIN_PARALLEL and p["L"] > 0)
    fv.test_flat_poison(long_pass["L"] - 1)
    try:
        assert got_of(fv.decode_full(ob, n, D.MODE_REFERENCE)) == want
        st = fv.stats()
    finally:
        fv.test_flat_poison(-1)
    assert st["flat_first_miss"] >= 1 and st["flat_missed"] >= 1
    # the speculative walks count, committed or not, and so do the ones that replaced them (no noise: every long walk retries)
    print(f"  poisoned at {long_pass['L'] - 1}: first miss {st['flat_first_miss']}, retries {st['bt_restarts']}")
    assert st["bt_restarts"] > on["bt_restarts"] if noise == 0 else st["bt_restarts"] > 0


# ---------------------------------------------------------------- 4. circulant ties, full-state

@pytest.mark.parametrize("last", [8, 9])
@pytest.mark.parametrize("T", [41, 130])
@pytest.mark.parametrize("K", [257, 1025, 2053])
def test_circulant_ties_full_state(ctx, K, T, last):
    A, Bm, Pi, om = circulant_model(K)
    ob = modelgen.circulant_observations(T, last, T)
    check_circulant(K, T, last)           # the model is what it claims, from the oracle's tables, before the GPU is judged
    path, score, restarts = whole_pass(om, ob)
    wants = {}
    for n in (1, 2, 3, 4, 7, 8):
        opath, oscore, _, orc = om.full_decode(ob, n)
        wants[n] = (opath.tolist(), bits(oscore), orc)
        assert orc == 0 and opath[-1] == modelgen.CIRCULANT_CUT[K][last - 8]
    runs = [(dense_ctx(ctx, ("circulant", K), A, Bm, Pi), k) for k in DENSE_KERNELS]
    runs += [(sparse_ctx(ctx, ("circulant", K), A, Bm, Pi), k) for k in (D.KERNEL_AUTO, D.KERNEL_CSR_F64)]
    for fv, kernel in runs:
        fv.set_option(D.OPT_KERNEL, kernel)
        assert got_of(fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)) == (path, score, 0), kernel
        assert fv.stats()["bt_restarts"] == restarts, kernel
        for n, want in wants.items():
            assert got_of(fv.decode_full(ob, n, D.MODE_REFERENCE)) == want, (kernel, n)
            assert fv.stats()["column_steps"] > 0, (kernel, n)


# ---------------------------------------------------------------- 3. batch

def test_batch_rotor_ragged_lengths(ctx):
    K, noise = 61, 0
    A, Bm, Pi, om = rotor_model(K, noise)
    obs = [observations(7, T, 2000 + T) for T in (40, 129, 2050, 2)]
    fv = dense_ctx(ctx, ("rotor", K, noise), A, Bm, Pi)
    fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
    single = [whole_pass(om, ob) for ob in obs]
    paths, scores, statuses = fv.decode_full_batch(obs, 1, D.MODE_SINGLE_PASS)
    assert [(p.tolist(), bits(s), 0) for p, s in zip(paths, scores)] == [(p, s, 0) for p, s, _ in single] and not statuses.any()
    assert fv.stats()["bt_restarts"] == sum(r for _, _, r in single) > 0
    for n in (1, 2, 4):
        want = []
        for ob in obs:
            opath, oscore, _, orc = om.full_decode(ob, n)
            want.append((opath.tolist(), bits(oscore), orc))
        paths, scores, statuses = fv.decode_full_batch(obs, n, D.MODE_REFERENCE)
        assert [(p.tolist(), bits(s), int(rc)) for p, s, rc in zip(paths, scores, statuses)] == want, n
        assert fv.stats()["bt_restarts"] >= sum(r for _, _, r in single), n


def test_batch_circulant_end_picks_in_one_launch(ctx):
    """three end picks of one final_argmax_batch launch: beyond the first trip of the loop, inside it past the first waves,
    and state 0"""
    K = 2053
    A, Bm, Pi, om = circulant_model(K)
    obs = [modelgen.circulant_observations(T, last, T) for T, last in ((41, 8), (130, 9), (24, 3))]
    fv = dense_ctx(ctx, ("circulant", K), A, Bm, Pi)
    single = [whole_pass(om, ob) for ob in obs]
    ends = [p[-1] for p, _, _ in single]
    assert ends[0] >= 1024 and 256 <= ends[1] < 1024 and ends[2] == 0
    for kernel in (D.KERNEL_F64_STREAM, D.KERNEL_AUTO):
        fv.set_option(D.OPT_KERNEL, kernel)
        paths, scores, statuses = fv.decode_full_batch(obs, 1, D.MODE_SINGLE_PASS)
        assert [(p.tolist(), bits(s)) for p, s in zip(paths, scores)] == [(p, s) for p, s, _ in single] and not statuses.any()
        for n in (2, 4):
            want = []
            for ob in obs:
                opath, oscore, _, orc = om.full_decode(ob, n)
                want.append((opath.tolist(), bits(oscore), orc))
            paths, scores, statuses = fv.decode_full_batch(obs, n, D.MODE_REFERENCE)
            assert [(p.tolist(), bits(s), int(rc)) for p, s, rc in zip(paths, scores, statuses)] == want, (kernel, n)
            assert [p[-1] for p in paths] == ends and fv.stats()["column_steps"] > 0


# ---------------------------------------------------------------- 5. beam

def beam_whole_pass(om, ob, beam):
    """the plain beam pass over the sequence from the oracle: (path, score bits, retries of the walk on its arg table)"""
    T = len(ob)
    _, arg, _, _, end, score = om.beam_forward(ob, 0, T - 1, -1, beam)
    table = arg.tolist()
    chain = btm.serial_walk(table, 0, T - 1, end)
    walked, restarts = btm.chunk_walk(table, 0, T - 1, end)
    assert walked == chain
    return chain + [end], bits(score), restarts


@pytest.mark.parametrize("T", [129, 2050])
@pytest.mark.parametrize("beam", [2, 64, 257])
@pytest.mark.parametrize("noise", [0, 0.02])
def test_rotor_beam(ctx, noise, beam, T):
    K = 257
    A, Bm, Pi, om = rotor_model(K, noise)
    ob = observations(7, T, 1000 + T)
    fv = dense_ctx(ctx, ("rotor", K, noise), A, Bm, Pi)
    path, score, restarts = beam_whole_pass(om, ob, beam)
    miss = min(path) < 0
    print(f"rotor K={K} noise={noise} B={beam} T={T}: the whole pass's walk retries {restarts} times, miss {miss}")
    assert restarts > 0
    for dbg in (0, EAGER_LAYOUTS):
        fv.set_option(D.OPT_DEBUG, dbg)
        got = got_of(fv.decode_beam(ob, 1, beam, D.MODE_SINGLE_PASS))
        st = fv.stats()
        assert got == (path, score, D.WARN_BEAM_MISS if miss else 0), dbg
        # no cell of this path is tied (beam_ties == 0): one walk, on the pointers the oracle has
        assert st["bt_restarts"] == restarts if st["beam_ties"] == 0 else st["bt_restarts"] >= restarts, (dbg, st["bt_restarts"], st["beam_ties"])
        for n in (1, 4):
            opath, oscore, _, orc = om.beam_decode(ob, n, beam, check=False)
            got = got_of(fv.decode_beam(ob, n, beam, D.MODE_REFERENCE))
            st = fv.stats()
            assert got == (opath.tolist(), bits(oscore), orc), (dbg, n)
            assert st["bt_restarts"] >= restarts, (dbg, n, st["bt_restarts"])


TIE_SPEC = dict(kind="ties_semi", K=96, M=8, seed=1, T=4161)
TIE_BEAM = 16


def test_beam_ties_and_retries_in_one_decode(ctx):
    """ties_semi K = 96 at T = 2049 and 4161, B = 16: on the oracle's beam arg table the walk of the whole pass retries 16
    and 17 times, and the decoded path runs through cells whose maximum two beam entries attained (beam_ties > 0): the
    tags must be counted on verified chunks only, the layouts rebuilt and the second walk retried as well."""
    A, Bm, Pi, ob = modelgen.model32(TIE_SPEC)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = dense_ctx(ctx, ("ties_semi", 96), A, Bm, Pi)
    seqs = [ob[:2049], ob]
    try:
        wants = {}
        for q, o in enumerate(seqs):
            path, score, restarts = beam_whole_pass(om, o, TIE_BEAM)
            assert restarts > 0
            for dbg in (0, EAGER_LAYOUTS):
                fv.set_option(D.OPT_DEBUG, dbg)
                got = got_of(fv.decode_beam(o, 1, TIE_BEAM, D.MODE_SINGLE_PASS))
                st = fv.stats()
                print(f"ties_semi T={len(o)} B={TIE_BEAM} debug={dbg}: beam_ties {st['beam_ties']} bt_restarts {st['bt_restarts']} (second walk alone: {restarts})")
                assert got == (path, score, 0), (q, dbg)
                assert st["beam_ties"] > 0 and st["bt_restarts"] >= restarts > 0, (q, dbg)
                for n in (1, 4):
                    opath, oscore, _, orc = om.beam_decode(o, n, TIE_BEAM, check=False)
                    wants[q, n] = (opath.tolist(), bits(oscore), orc)
                    got = got_of(fv.decode_beam(o, n, TIE_BEAM, D.MODE_REFERENCE))
                    st = fv.stats()
                    assert got == wants[q, n], (q, dbg, n)
                    assert st["beam_ties"] > 0 and st["bt_restarts"] >= restarts, (q, dbg, n)
        fv.set_option(D.OPT_DEBUG, 0)
        for n in (1, 4):
            paths, scores, statuses = fv.decode_beam_batch(seqs, n, TIE_BEAM, D.MODE_REFERENCE)
            st = fv.stats()
            assert [(p.tolist(), bits(s), int(rc)) for p, s, rc in zip(paths, scores, statuses)] == [wants[0, n], wants[1, n]], n
            assert st["beam_ties"] > 0 and st["bt_restarts"] > 0, n
    finally:
        om.close()


def test_beam_tag_on_an_unverified_chunk_does_not_count(ctx):
    """rotor_tied_column, K = B = 131, T = 129, the one symbol 1 placed so that the true chain passes the tied column at a
    time when it is not tied.  The chain of 128 steps is walked by 64 lanes; in one round a lane that started from a wrong
    guess runs through the column at a time when it IS tied, on a chunk that then fails its check.  That tag is not on
    the decoded path: the lazy decode must finish without rebuilding the layouts (beam_ties == 0).  The tied cells and the
    two verdicts come from the oracle's tables and tests/backtrack_model.py."""
    K, g, T, u = 131, 30, 129, 27
    A, Bm, Pi = modelgen.rotor_tied_column(K, g)
    ob = np.zeros(T, dtype=np.int32)
    ob[u] = 1
    om = oracle.OracleModel(A, Bm, Pi)
    fv = dense_ctx(ctx, ("rotor_tied_column", K), A, Bm, Pi)
    try:
        scores, arg, _, _, end, fscore = om.beam_forward(ob, 0, T - 1, -1, K)
        # (B = K: every state is in every heap; all log A are 0: a column's candidates are its predecessors' scores)
        tagged = {(t, g + 1) for t in range(1, T) if scores[t - 1][g] == scores[t - 1][g - 1]}
        chain, restarts, on_path, anywhere = btm.chunk_walk_tags(arg.tolist(), 0, T - 1, end, tagged)
        assert chain == btm.serial_walk(arg.tolist(), 0, T - 1, end) and g + 1 in chain
        assert len(tagged) >= T - 4 and restarts > 0 and anywhere and not on_path          # the case is what it claims
        want = (chain + [end], bits(fscore), 0)
        for mode in (D.MODE_SINGLE_PASS, D.MODE_REFERENCE):
            fv.set_option(D.OPT_DEBUG, 0)
            if mode == D.MODE_REFERENCE:
                opath, oscore, _, orc = om.beam_decode(ob, 1, K, check=False)
                want = (opath.tolist(), bits(oscore), orc)
            assert got_of(fv.decode_beam(ob, 1, K, mode)) == want, mode
            st = fv.stats()
            print(f"tied column off the path, mode {mode}: beam_ties {st['beam_ties']} bt_restarts {st['bt_restarts']} (model {restarts})")
            if mode == D.MODE_SINGLE_PASS:
                assert st["beam_ties"] == 0 and st["bt_restarts"] == restarts
            fv.set_option(D.OPT_DEBUG, EAGER_LAYOUTS)
            assert got_of(fv.decode_beam(ob, 1, K, mode)) == want, mode
            assert fv.stats()["beam_ties"] > 0          # the tags are there: rebuilt when asked for
    finally:
        om.close()


# ---------------------------------------------------------------- 6. a dead end at parallel length

def test_dead_end_at_parallel_length(ctx):
    """The band that ends (tests/test_gpu_row_codes.py) stretched to T = 200: the last row has no finite score, the end pick
    is state 0 of a dead row and its chain of 199 steps — walked by 64 lanes — is -1 from the first hop on.  (A live end's
    chain cannot die midway: a live cell has a live predecessor.)  The oracle's decode answers FV_ERR_NO_PRED too; what it
    leaves in the path then is the reference's undefined read, so the entries are judged on its arg table."""
    T = 200
    A, Bm, Pi, ob = band_model(48, 2, 4, T, 32, dead_end=True)
    om = oracle.OracleModel(A, Bm, Pi)
    fv = dense_ctx(ctx, ("band", 48), A, Bm, Pi)
    try:
        row, args = om.full_forward(ob, 0, T - 1, -1)
        assert (row <= -np.finfo(np.float32).max).all() and (args[-1] == -1).all()
        end = int(np.argmax(row))
        want = btm.serial_walk(args.tolist(), 0, T - 1, end) + [end]
        assert want == [-1] * (T - 1) + [0]
        for kernel in (D.KERNEL_F64_STREAM, D.KERNEL_U16_REFINE):
            fv.set_option(D.OPT_KERNEL, kernel)
            for n in (1, 4):
                orc = om.full_decode(ob, n, check=False)[3]
                path, score, rc = raw_full(fv, ob, n)
                st = fv.stats()
                assert rc == orc == D.ERR_NO_PRED, (kernel, n, rc, orc)
                assert path == want and score == bits(row[end]), (kernel, n)
                assert st["bt_restarts"] == 0          # (dead chunks agree with one another: -1 entered, -1 left)
        fv.set_option(D.OPT_KERNEL, D.KERNEL_F64_STREAM)
        with pytest.raises(decoder.FlashVitError) as err:
            fv.decode_full(ob, 1, D.MODE_SINGLE_PASS)
        assert err.value.rc == D.ERR_NO_PRED and om.vanilla_decode(ob, check=False)[2] == D.ERR_NO_PRED
    finally:
        om.close()
