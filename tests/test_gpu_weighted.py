"""GPU (-m gpu): weighted hand ranges (rs_best_response_weighted, rs_node_report_weighted, rs_range_cfr_create_weighted) against the numpy restatement
tests/np_weighted.py, on the three cases of tests/test_weighted_cpu.py (a river, a turn and a flop start; weights rng.integers(1, 9) / 4).

np_br.best_response, np_range_cfr.sweep and np_node_report.report run unchanged on a WeightedGame; the device is held to them within RTOL, ATOL of test_np_br_cpu
("two summation orders of the same f64 sums"), a swept table's cells to test_range_cfr_cpu.compare_cells (one f32 ulp or ATOL).  BR_MAX is discontinuous where two
actions nearly tie: check_margins is asserted on every comparison (the restatement alone says the cases are clear of rounding: test_weighted_cpu prints the margins).
Beside the restatement: unit weights are the unweighted call bit for bit; weights scaled by 2 and 0.5 change no bit; integer weights are repeated hands; the two
distributions agree where N0 and N1 are constant and differ where they are not; what the header refuses is refused with nothing written; the wrapper's zero weights."""
import ctypes as C

import numpy as np
import pytest

import np_node_report as nnr
import np_range_cfr as nrc
import np_weighted as nw
import rustsolver_amd as rs
from oracle import np_br as nbr
from rustsolver_amd import _lib as L
from test_gpu_br_pinned import depth_first
from test_gpu_node_report import action_ids, same_reports
from test_gpu_node_report import compare as compare_reports
from test_gpu_range_cfr import Device, compare_sweep, copy_tables, same_tables
from test_np_br_cpu import ATOL, RIVER, RTOL, check_margins, combos_of, random_cids
from test_range_cfr_cpu import random_tables
from test_weighted_cpu import CASES, game_of, make_case, strategies_of, tables_of

pytestmark = pytest.mark.gpu
GDT = {"i32": L.I32, "f32": L.F32}
DEAL = {"sequential": L.DEAL_SEQUENTIAL, "joint": L.DEAL_JOINT}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if rs.device_count() < 1:
        pytest.fail("no HIP device visible: GPU parity tests need a real MI355X (there is no CPU fallback)")


def device_of(case, dtype="f32", tables=None):
    dev = Device(case["board0"], case["h"], case["cids"], case["sizes"], case["tree"], dtype=GDT[dtype])
    assert dev.tree.n_nodes == len(case["nodes"])
    dev.upload(*(tables or tables_of(case, dtype)))
    return dev


def br(dev, mode, weights=None, deal="sequential", h=None, cids=None):
    h, cids = h or dev.h, cids or dev.cids
    return dev.table.best_response_rounds(dev.tree, dev.board0, h[0], h[1], cids, mode, weights=weights, deal=deal)


def report(dev, p, ids, weights=None, deal="sequential", **kw):
    return dev.table.node_report(dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, p, ids, weights=weights, deal=deal, **kw)


def solver(dev, weights=None, deal="sequential", **kw):
    return rs.RangeCFR(dev.table, dev.tree, dev.board0, dev.h[0], dev.h[1], dev.cids, weights=weights, deal=deal, **kw)


def close(got, want, what):
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL), (what, got, want)


# ---- 1. best response against the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["i32", "f32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_best_response_equals_the_restatement(name, dtype):
    case = make_case(name)
    tables = tables_of(case, dtype)
    dev = device_of(case, dtype, tables)
    for deal in nw.DEALS:
        game = game_of(case, deal)
        for current in (False, True):                              # the current strategies once: rank-order leaves only
            sig = strategies_of(tables, current, dtype)
            margins = []
            want = {L.BR_MAX: nbr.best_response(case["nodes"], sig.__getitem__, None, None, case["cids"], "max", margins, game),
                    L.BR_AVERAGE: nbr.best_response(case["nodes"], sig.__getitem__, None, None, case["cids"], "avg", None, game)}
            check_margins(margins)
            assert abs(want[L.BR_AVERAGE].sum()) < 1e-9
            for mode in (L.BR_MAX, L.BR_AVERAGE):
                for bits in ((L.BR_SORTED | L.BR_CURRENT,) if current else (0, L.BR_SORTED)):
                    got = br(dev, mode | bits, case["w"], deal)
                    print(name, dtype, deal, hex(mode | bits), got, want[mode])
                    close(got, want[mode], (name, dtype, deal, mode | bits))
                    if mode == L.BR_AVERAGE:
                        assert abs(got.sum()) < 1e-9, (name, dtype, deal, bits, got)
            if not current:
                for bits in (0, L.BR_SORTED):
                    real = br(dev, L.BR_MAX | L.BR_REAL | bits, case["w"], deal)
                    assert (real >= br(dev, L.BR_MAX | bits, case["w"], deal) - 1e-9).all(), (name, dtype, deal, bits, real)
    dev.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_real_game_equals_the_abstract_one_where_every_lane_is_an_info_set(name):
    """one info set per (prefix, hand): the abstraction's responder sees what the real game's sees.  No margin is asserted here: an info set of a few lanes whose actions
    are worth the same but for rounding (the flop case has one 2.7e-19 of its node's scale apart) may go either way in either reading, and with perfect recall the choice
    moves the total by that margin alone -- far inside RTOL"""
    case = make_case(name, lanes=True)
    tables = tables_of(case, "i32")
    dev = device_of(case, "i32", tables)
    sig = strategies_of(tables, False, "i32")
    for deal in nw.DEALS:
        want = nbr.best_response(case["nodes"], sig.__getitem__, None, None, case["cids"], "max", None, game_of(case, deal))
        for bits in (0, L.BR_SORTED):
            plain, real = br(dev, L.BR_MAX | bits, case["w"], deal), br(dev, L.BR_MAX | L.BR_REAL | bits, case["w"], deal)
            close(plain, want, (name, deal, bits))
            assert (real >= plain - 1e-9).all() and np.allclose(real, plain, rtol=RTOL, atol=0), (name, deal, bits, real, plain)
    dev.close()


# ---- 2. and 3. unit weights, scaled weights ---------------------------------------------------------------------------------------------------------------
ALL_MODES = [m | s | c for m in (L.BR_MAX, L.BR_AVERAGE) for s in (0, L.BR_SORTED) for c in (0, L.BR_CURRENT)] + [L.BR_MAX | L.BR_REAL, L.BR_MAX | L.BR_REAL | L.BR_SORTED]


def everything(dev, case, before, weights, sweeps):
    """out[] in every mode, every row of both traversers' reports (average and current), and the tables after `sweeps` full-width iterations from `before`"""
    ids = action_ids(case["nodes"])
    dev.upload(*before)
    outs = [br(dev, m, weights) for m in ALL_MODES]
    reports = [report(dev, p, ids, weights, current=c, sorted_showdowns=s) for p in (0, 1) for c in (False, True) for s in (True, False)]
    s = solver(dev, weights)
    values = [s.iterate(p) for _ in range(sweeps) for p in (0, 1)]
    s.destroy()
    return outs, reports, values, dev.download()


def same_everything(a, b, what):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])), (what, "out[]", a[0], b[0])
    assert all(same_reports(x, y) for x, y in zip(a[1], b[1])), (what, "report")
    assert a[2] == b[2], (what, "values", a[2], b[2])
    assert same_tables(a[3], b[3]), (what, "tables")


@pytest.mark.parametrize("name", sorted(CASES))
def test_unit_weights_are_the_unweighted_call_bit_for_bit(name):
    case = make_case(name)
    before = tables_of(case, "f32")
    dev = device_of(case, "f32", before)
    n0, n1 = len(case["h"][0]), len(case["h"][1])
    plain = everything(dev, case, before, None, 2)
    assert not same_tables(plain[3], before)
    for weights in ((np.ones(n0), np.ones(n1)), (np.ones(n0), None), (None, np.ones(n1))):
        same_everything(everything(dev, case, before, weights, 2), plain, (name, [w is None for w in weights]))
    dev.close()


@pytest.mark.parametrize("deal", nw.DEALS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_scaling_one_range_up_and_the_other_down_changes_no_bit(name, deal):
    case = make_case(name)
    before = tables_of(case, "f32")
    dev = device_of(case, "f32", before)
    ids = action_ids(case["nodes"])

    def run(weights):
        dev.upload(*before)
        outs = [br(dev, m, weights, deal) for m in ALL_MODES]
        reports = [report(dev, p, ids, weights, deal, sorted_showdowns=s) for p in (0, 1) for s in (True, False)]
        s = solver(dev, weights, deal)
        values = [s.iterate(0), s.iterate(1)]
        s.destroy()
        return outs, reports, values, dev.download()

    same_everything(run((case["w"][0] * 2.0, case["w"][1] * 0.5)), run(case["w"]), (name, deal))
    dev.close()


# ---- 4. integer weights are repeated hands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_integer_weights_are_repeated_hands_on_the_device(name):
    """pair loop: RS_BR_SORTED takes ranges of distinct combos"""
    case = make_case(name)
    dev = device_of(case, "i32")
    k = np.random.Generator(np.random.PCG64(case["seed"] + 7)).integers(1, 4, len(case["h"][1]))
    hands, cids = nw.repeat_hands(case["h"], case["cids"], 1, k)
    for deal in nw.DEALS:
        for mode in (L.BR_MAX, L.BR_AVERAGE):
            weighted = br(dev, mode, (None, k.astype(np.float64)), deal)
            listed = br(dev, mode, None, deal, h=hands, cids=cids)
            close(weighted, listed, (name, deal, mode))
    with pytest.raises(rs.RsError):
        br(dev, L.BR_MAX | L.BR_SORTED, None, "joint", h=hands, cids=cids)
    dev.close()


# ---- 5. full-width CFR ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deal", nw.DEALS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_sweep_equals_the_restatement(name, deal):
    case = make_case(name)
    game = game_of(case, deal)
    dev = device_of(case, "f32")
    cells = differ = 0
    for rmplus in (False, True):
        s = solver(dev, case["w"], deal, rmplus=rmplus)
        assert s.nbytes > 0
        for p in (0, 1):
            before = random_tables(np.random.Generator(np.random.PCG64(case["seed"] + 2 * p + rmplus)), case["nodes"], case["sizes"])
            want = copy_tables(*before)
            value = nrc.sweep(case["nodes"], want[0], want[1], game, case["cids"], p, rmplus)
            dev.upload(*before)
            got_value = s.iterate(p)
            got = dev.download()
            print(name, deal, rmplus, p, got_value, value)
            assert np.isclose(got_value, value, rtol=RTOL, atol=ATOL), (name, deal, rmplus, p, got_value, value)
            c, d, _ = compare_sweep(case["nodes"], game, case["cids"], p, before, got, want, (name, deal, rmplus, p))
            cells, differ = cells + c, differ + d
        s.destroy()
    assert cells > 0 and differ <= 0.005 * cells, (name, deal, differ, cells)
    dev.close()


@pytest.mark.parametrize("name", ["TURN", "FLOP"])
def test_level_plan_and_depth_first_walk_give_the_same_bits(name):
    case = make_case(name)
    before = tables_of(case, "f32")
    dev = device_of(case, "f32", before)
    for deal in nw.DEALS:
        for rmplus in (False, True):
            dev.upload(*before)
            levels = solver(dev, case["w"], deal, rmplus=rmplus)
            v = [levels.iterate(0), levels.iterate(1)]
            assert levels.launches() > 0
            got = dev.download()
            levels.destroy()
            with depth_first():
                walk = solver(dev, case["w"], deal, rmplus=rmplus)
                dev.upload(*before)
                w = [walk.iterate(0), walk.iterate(1)]
                assert walk.launches() == -1
            assert v == w, (name, deal, rmplus, v, w)
            assert same_tables(dev.download(), got), (name, deal, rmplus)
            walk.destroy()
    dev.close()


# ---- 6. node report ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_report_equals_the_restatement(name):
    case = make_case(name)
    tables = tables_of(case, "f32")
    dev = device_of(case, "f32", tables)
    ids = action_ids(case["nodes"])
    root = ids[0]
    assert root == min(ids) and not any(case["nodes"][i]["kind"] == "action" for i in range(root))
    for deal in nw.DEALS:
        game = game_of(case, deal)
        for p in (0, 1):
            for current in (False, True):
                want = nnr.report(case["nodes"], nnr.strategies(tables, current, "f32").__getitem__, game, case["cids"], p)
                for sorted_showdowns in (True, False):
                    got = report(dev, p, ids, case["w"], deal, current=current, sorted_showdowns=sorted_showdowns)
                    compare_reports(got, want, (name, deal, p, current, sorted_showdowns))
                    if deal == "joint":
                        assert abs(got[root]["mass"].sum() - 1.0) < 1e-12, (name, p, got[root]["mass"].sum())
    dev.close()


# ---- 7. the two distributions ---------------------------------------------------------------------------------------------------------------------------
def test_joint_is_sequential_where_the_counts_are_constant():
    """a full board and both ranges all 1 081 combos: N0 = 1 081 and N1 = 990 on every lane, so the two distributions are one; on the 40 / 47 ranges they are not"""
    case = make_case("RIVER")
    full = combos_of(RIVER)
    assert len(full) == 1081
    h = [full, full]
    cids = random_cids(np.random.Generator(np.random.PCG64(5)), RIVER, h, case["sizes"])
    dev = device_of(case, "i32")
    for mode in (L.BR_MAX, L.BR_AVERAGE, L.BR_MAX | L.BR_SORTED, L.BR_AVERAGE | L.BR_SORTED):
        seq, joint = br(dev, mode, None, "sequential", h=h, cids=cids), br(dev, mode, None, "joint", h=h, cids=cids)
        close(joint, seq, ("full ranges", mode))
        assert seq.tobytes() == br(dev, mode, h=h, cids=cids).tobytes()
        seq, joint = br(dev, mode, None, "sequential"), br(dev, mode, None, "joint")
        assert not np.allclose(joint, seq, rtol=1e-6, atol=1e-9), ("40 / 47", mode, seq, joint)
    dev.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refused_weights_leave_everything_alone():
    case = make_case("TURN")
    dev = device_of(case, "f32")
    lib = L.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    b = np.ascontiguousarray(dev.board0, dtype=np.uint8)
    h = [np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 2) for x in dev.h]
    keep = [np.ascontiguousarray(dev.cids[r][p], dtype=np.uint32) for r in range(len(dev.cids)) for p in (0, 1)]
    arr = (C.c_void_p * len(keep))(*[k.ctypes.data for k in keep])
    ids = np.asarray(action_ids(case["nodes"]), dtype=np.int32)
    game = (dev.table._h, dev.tree._h, vp(b), len(b), vp(h[0]), len(h[0]), vp(h[1]), len(h[1]), arr, len(dev.cids))
    checksum = dev.table.checksum()

    def struct(w0, w1, deal=L.DEAL_SEQUENTIAL, reserved=0):
        rw = L.RangeWeights()
        rw.w[0], rw.w[1], rw.deal, rw.reserved = w0.ctypes.data, w1.ctypes.data, deal, reserved
        return rw

    good = [np.ascontiguousarray(w) for w in case["w"]]
    refused = {}
    for what, bad in (("NaN", np.nan), ("+inf", np.inf), ("0.0", 0.0), ("negative", -0.25), ("-inf", -np.inf)):
        for p in (0, 1):
            w = [x.copy() for x in good]
            w[p][len(w[p]) // 2] = bad
            refused[what, p] = (w, struct(w[0], w[1]))
    refused["deal = 2"] = (good, struct(good[0], good[1], deal=2))
    refused["deal = -1"] = (good, struct(good[0], good[1], deal=-1))
    refused["reserved = 1"] = (good, struct(good[0], good[1], reserved=1))
    huge = [np.full(len(good[0]), 1.7e308), good[1]]
    refused["a sum that overflows"] = (huge, struct(huge[0], huge[1]))
    total = int(lib.rs_node_report_size(dev.tree._h, len(b), len(h[0]), vp(ids), len(ids), None))
    for what, (w, rw) in refused.items():
        for mode in (L.BR_MAX, L.BR_AVERAGE | L.BR_SORTED):
            out = np.full(2, 7.0)
            assert lib.rs_best_response_weighted(*game, C.byref(rw), mode, out.ctypes.data_as(C.POINTER(C.c_double))) == L.ERR_INVALID, what
            assert (out == 7.0).all() and b"rs_range_weights" in lib.rs_last_error(), what
        buf = np.full(total, 7.0)
        assert lib.rs_node_report_weighted(*game, C.byref(rw), L.BR_AVERAGE, 0, vp(ids), len(ids), vp(buf), len(buf)) == L.ERR_INVALID, what
        assert (buf == 7.0).all(), what
        handle = C.c_void_p()
        assert lib.rs_range_cfr_create_weighted(*game, C.byref(rw), None, C.byref(handle)) == L.ERR_INVALID, what
        assert not handle.value, what
        assert dev.table.checksum() == checksum, what
    with pytest.raises(rs.RsError) as e:
        solver(dev, (good[0], -good[1]))
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(rs.RsError) as e:
        br(dev, L.BR_MAX, good, deal=2)
    assert e.value.code == L.ERR_INVALID
    assert dev.table.checksum() == checksum
    rw = struct(good[0], good[1], deal=L.DEAL_JOINT)                # the same arguments with nothing wrong
    out = np.full(2, 7.0)
    assert lib.rs_best_response_weighted(*game, C.byref(rw), L.BR_MAX, out.ctypes.data_as(C.POINTER(C.c_double))) == L.OK and not (out == 7.0).any()
    dev.close()


# ---- 9. the wrapper's zero weights --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deal", nw.DEALS)
def test_a_zero_weight_takes_the_hand_out_of_the_range(deal):
    case = make_case("TURN")
    before = tables_of(case, "f32")
    dev = device_of(case, "f32", before)
    ids = action_ids(case["nodes"])
    w = [x.copy() for x in case["w"]]
    w[0][[0, 32]] = 0.0                                             # three hands: the first and the last of player 0, one of player 1
    w[1][[5]] = 0.0
    stay = [x != 0 for x in w]
    h = [dev.h[p][stay[p]] for p in (0, 1)]
    cids = [[np.asarray(row[p])[:, stay[p]] for p in (0, 1)] for row in dev.cids]
    ws = [w[p][stay[p]] for p in (0, 1)]
    for mode in (L.BR_MAX, L.BR_AVERAGE, L.BR_MAX | L.BR_SORTED):
        close(br(dev, mode, w, deal), br(dev, mode, ws, deal, h=h, cids=cids), (deal, mode))
    for p in (0, 1):
        got = report(dev, p, ids, w, deal)
        want = dev.table.node_report(dev.tree, dev.board0, h[0], h[1], cids, p, ids, weights=ws, deal=deal)
        for i in ids:
            for key in ("cfv", "value", "mass", "own"):
                assert got[i][key].shape[-1] == len(dev.h[p])
                assert (got[i][key][..., ~stay[p]] == 0.0).all(), (deal, p, i, key)
                close(got[i][key][..., stay[p]], want[i][key], (deal, p, i, key))
    a, b = solver(dev, w, deal), rs.RangeCFR(dev.table, dev.tree, dev.board0, h[0], h[1], cids, weights=ws, deal=deal)
    dev.upload(*before)
    va = [a.iterate(0), a.iterate(1)]
    ta = dev.download()
    dev.upload(*before)
    assert [b.iterate(0), b.iterate(1)] == va and same_tables(dev.download(), ta)
    a.destroy()
    b.destroy()
    dev.close()
