"""Rake on the deal path, restated for the numpy walk (oracle/np_walk.iterate_deals) without touching it: a raked leaf IS a utility row.

iterate_deals takes ("util", buf) leaves verbatim, but pays an uncontested terminal +-value itself.  So every terminal of the tree's records is retyped to a showdown
terminal and given, per traverser, the f32 row the rake implies: win / tie / lose selected by the deal's sign at a showdown or all-in, the one constant at an uncontested
terminal.  The numbers are rustsolver_amd.rake.payoffs' (rs_rake_payoffs, f64), each cast to float32 once -- what the raked deal solver puts into its kernels' constants.

The same retyped records, built into a tree (tree_from_nodes) and given LEAF_UTIL buffers of these rows, run the device's UNRAKED deal solver on the raked game: a second
yardstick, independent of numpy.  Pure numpy apart from rake.payoffs and tree_from_nodes.
"""
import ctypes as C

import numpy as np

import rustsolver_amd as rs
from oracle import np_walk as npw
from rustsolver_amd import _lib as L
from rustsolver_amd import rake as raked

F32 = np.float32


def retyped_records(tree):
    """the tree's node records with every terminal typed SHOWDOWN (copies; value, last_to_act and round as they were)"""
    out = []
    for nd in tree.nodes:
        c = L.TreeNode()
        C.memmove(C.byref(c), C.byref(nd), C.sizeof(L.TreeNode))
        if c.kind == L.NODE_TERMINAL:
            c.ttype = L.TERM_SHOWDOWN
        out.append(c)
    return out


def retyped_nodes(tree):
    """np_walk's node dicts of the retyped records"""
    return npw.tree_from_records(retyped_records(tree))


def retyped_tree(tree):
    """the retyped records as a GameTree (same node ids, same action indices)"""
    return rs.tree_from_nodes(retyped_records(tree))


def terminals(tree):
    return [i for i, nd in enumerate(tree.nodes) if nd.kind == L.NODE_TERMINAL]


def util_rows(tree, rake, sign, player):
    """{terminal id: float32 [n_deals]}: what traverser `player` is paid at every terminal of `tree` (the ORIGINAL tree: its terminal types decide) under rake
    (None = unraked) on deals whose showdown sign row (sign(score0 - score1)) is `sign`"""
    x = np.asarray(sign, dtype=F32)
    wins = x > 0 if player == 0 else x < 0
    rows = {}
    for i in terminals(tree):
        win, tie, lose = (F32(v) for v in raked.payoffs(tree, i, rake, player))
        if tree.nodes[i].ttype == L.TERM_UNCONTESTED:
            rows[i] = np.full(len(x), win, dtype=F32)
        else:
            rows[i] = np.where(x == 0, tie, np.where(wins, win, lose)).astype(F32)
    return rows


def util_leaves(tree, rake, sign, player):
    """np_walk's `leaves` of traverser `player` for the retyped nodes"""
    return {i: ("util", row) for i, row in util_rows(tree, rake, sign, player).items()}


def capped_terminals(tree, rake):
    """(terminals whose rake is the cap, terminals whose rake is rate * pot): r = min(cap, rate * pot), pot = float32(value)"""
    capped, free = [], []
    for i in terminals(tree):
        pot = float(F32(tree.nodes[i].value))
        (capped if rake[0] * pot > rake[1] else free).append(i)
    return capped, free
