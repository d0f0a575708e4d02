"""Rake (include/rustsolver_amd.h, rs_rake), restated in numpy from its definition on oracle/np_br.py's Game.

TEST INFRASTRUCTURE ONLY.  Written from the definition and np_br's dense deal matrices, not from the device code: no tie mass, no prefix sums, no rank order.  The
walks are tests/np_locks.py's -- best response in every mode, the sweep and train, the report, the second summation order -- which take every leaf from _Walk.terminal
and stay as they are: for the duration of a call np_locks._Walk is this file's subclass, whose terminal() is the only thing that differs.

rake = None | (rate, cap).  For a terminal n: pot = float(float32(n.value)), r = min(cap, rate * pot), one f64 multiply.  Traverser p is paid
    UNCONTESTED            -pot if p folded (p == last_to_act), pot - r otherwise: the fold matrix W times that scalar
    SHOWDOWN, ALLIN        W * U, U = where(S > 0, vw, where(S < 0, vl, vt)) from the traverser's side, vw = pot - r, vl = -pot, vt = -0.5 * r
None, rate == 0 and cap == 0 are np_locks itself, to the bit.  Mass rows (report) are the fold matrix times 1.0: no terminal, not raked.
"""
import contextlib

import numpy as np

import np_locks as nl


def rake_of(nd, rake):
    """(pot, r) of a terminal node"""
    pot = float(np.float32(nd["value"]))
    return pot, (0.0 if rake is None else min(float(rake[1]), float(rake[0]) * pot))


def payoffs(nd, rake, p):
    """(win, tie, lose) of traverser p at terminal nd; an uncontested terminal: its one payoff three times"""
    pot, r = rake_of(nd, rake)
    if nd["ttype"] == "UNCONTESTED":
        u = -pot if p == nd["last_to_act"] else pot - r
        return u, u, u
    return pot - r, (-0.5 * r if r > 0.0 else 0.0), -pot


def is_raked(rake):
    return rake is not None and rake[0] > 0 and rake[1] > 0


class _RakedWalk(nl._Walk):
    rake = None                                                                     # set by _raked for the duration of a call

    def __init__(self, *args):
        super().__init__(*args)
        g = self.g
        sign, W = (g.S, g.W) if self.p == 0 else (-g.S.transpose(0, 2, 1), g.W.transpose(0, 2, 1))   # the traverser's side: [NB][n_p][n_o]
        if self.reverse:
            sign, W = sign[:, :, ::-1], W[:, :, ::-1]
        self.sign, self.Wp, self._M = sign, W, {}

    def terminal(self, nd, q):
        if not is_raked(self.rake):
            return super().terminal(nd, q)
        vw, vt, vl = payoffs(nd, self.rake, self.p)
        if nd["ttype"] == "UNCONTESTED":
            return self.leaf(self.M_fold, q) * vw
        if (vw, vt, vl) not in self._M:
            self._M[(vw, vt, vl)] = np.ascontiguousarray(self.Wp * np.where(self.sign > 0, vw, np.where(self.sign < 0, vl, vt)))
        return self.leaf(self._M[(vw, vt, vl)], q)


@contextlib.contextmanager
def _raked(rake):
    saved = nl._Walk
    _RakedWalk.rake = rake
    nl._Walk = _RakedWalk
    try:
        yield
    finally:
        nl._Walk = saved
        _RakedWalk.rake = None


def best_response(nodes, sigma, game, cids, mode="max", locks=None, reverse=False, real=False, rake=None):
    with _raked(rake):
        return nl.best_response(nodes, sigma, game, cids, mode, locks, reverse, real)


def sweep(nodes, R, S, game, cids, p, rmplus=False, locks=None, reverse=False, rake=None):
    with _raked(rake):
        return nl.sweep(nodes, R, S, game, cids, p, rmplus, locks, reverse)


def train(nodes, R, S, game, cids, iterations, rmplus=False, locks=None, rake=None):
    with _raked(rake):
        return nl.train(nodes, R, S, game, cids, iterations, rmplus, locks)


def report(nodes, sigma, game, cids, p, locks=None, reverse=False, rake=None):
    with _raked(rake):
        return nl.report(nodes, sigma, game, cids, p, locks, reverse)


def expected_rake(nodes, sigma, game, cids, rake, locks=None):
    """the rake the profile pays per deal, by a walk of its own: every terminal is an uncontested-style leaf of value r(n) -- the fold matrix on the opponent's reach --
    times the traverser's own reach, summed over the lanes and the terminals.  At a fold the folder pays nothing and the winner r, at a showdown the winner r or each
    player r / 2: r per deal that ends there, whoever wins"""
    w = nl._Walk(nodes, game, cids, 0, locks, False)
    total = 0.0

    def walk(i, q, pi):
        nonlocal total
        nd = nodes[i]
        if nd["kind"] == "terminal":
            total += float((pi * w.leaf(w.M_fold, q)).sum()) * rake_of(nd, rake)[1]
            return
        if nd["kind"] != "action":
            return walk(nd["children"][0], q, pi)
        sig = np.asarray(sigma(nd["index"]), dtype=np.float32).astype(np.float64)
        if nd["player"] != 0:
            so = w.opp_sigma(i, sig)
            for a, ch in enumerate(nd["children"]):
                walk(ch, q * so[a], pi)
            return
        sk = w.lanes(i)
        if sk is None:
            sk = sig[:, game.infoset_of(cids, nd["round_idx"], 0)]
        for a, ch in enumerate(nd["children"]):
            walk(ch, q, pi * sk[a])

    walk(0, np.ones((w.NB, game.n[1])), np.ones((w.NB, game.n[0])))
    return total


def exploitability(nodes, sigma, game, cids, rake, locks=None):
    """of the profile in the raked game, and the rake it pays: ((max0 - avg0) + (max1 - avg1)) / 2, -(avg0 + avg1)"""
    mx = best_response(nodes, sigma, game, cids, "max", locks, rake=rake)
    av = best_response(nodes, sigma, game, cids, "avg", locks, rake=rake)
    return ((mx[0] - av[0]) + (mx[1] - av[1])) / 2.0, -(av[0] + av[1])
