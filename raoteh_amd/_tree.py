"""
networkx tree -> flat arrays, exactly as the reference marshals them for its
native passes:

* BFS-directed tree + DFS preorder node list   raoteh/sampler/_mcy_dense.py:246-255
* children CSR in preorder index space          raoteh/sampler/_density.py:104-140
* per-edge matrices keyed by the CHILD index    raoteh/sampler/_density.py:143-180
"""
from __future__ import annotations

import numpy as np

__all__ = ['TreeArrays', 'marshal_tree', 'check_square_dense', 'nni_apply', 'place_apply',
           'spr_apply']


def check_square_dense(M):
    """Same checks and messages as raoteh/sampler/_density.py:79-101."""
    if M is None:
        raise ValueError('the matrix is None')
    try:
        shape = M.shape
    except AttributeError:
        if hasattr(M, 'number_of_nodes'):
            raise ValueError('expected an ndarray but found a graph object')
        raise ValueError('expected an ndarray')
    if len(shape) != 2:
        raise ValueError('expected len(M.shape) == 2')
    if shape[0] != shape[1]:
        raise ValueError('expected the array to be square')


class TreeArrays(object):
    """preorder_nodes, node_to_index, indices/indptr (int64 CSR of children),
    parent (int64, -1 at the root) and the nx edge data dict above each node."""

    def __init__(self, T, root):
        if root not in T:
            raise ValueError('the specified root is not in the tree')
        self.root = root
        # one depth-first walk in adjacency order: the preorder of
        # nx.dfs_preorder_nodes and, per node, the child order of nx.bfs_edges
        # (both follow the adjacency order; _density.py:104-140, _mcy_dense.py:255)
        adj = T._adj if hasattr(T, '_adj') else T.adj
        preorder, parent_of, children = [root], {root: None}, {root: []}
        stack = [(root, iter(adj[root]))]
        while stack:
            node, it = stack[-1]
            for nb in it:
                if nb in parent_of:
                    if nb != parent_of[node]:
                        raise ValueError('the graph is not a tree')
                    continue
                parent_of[nb] = node
                children[node].append(nb)
                children[nb] = []
                preorder.append(nb)
                stack.append((nb, iter(adj[nb])))
                break
            else:
                stack.pop()
        self.preorder_nodes = preorder
        n = len(preorder)
        if n != T.number_of_nodes():
            raise ValueError('the number of nodes is inconsistent')
        if T.number_of_edges() != n - 1:
            raise ValueError('the graph is not a tree')
        self.node_to_index = dict((v, i) for i, v in enumerate(preorder))
        self.parent = np.full(n, -1, dtype=np.int64)
        self.edge_data = [None] * n
        for ib in range(1, n):
            nb = preorder[ib]
            na = parent_of[nb]
            self.parent[ib] = self.node_to_index[na]
            self.edge_data[ib] = adj[na][nb]
        indices = []
        indptr = [0]
        for na in preorder:
            indices.extend(self.node_to_index[nb] for nb in children[na])
            indptr.append(len(indices))
        self.indices = np.array(indices, dtype=np.int64)
        self.indptr = np.array(indptr, dtype=np.int64)
        self.nnodes = n

    def branch_lengths(self):
        """f64[nnodes]: weight of the edge above each node (0 at the root)."""
        t = np.zeros(self.nnodes, dtype=np.float64)
        for i in range(1, self.nnodes):
            t[i] = self.edge_data[i]['weight']
        return t

    def rate_matrices(self, nstates, Q_default=None):
        """(Q f64[nq,n,n], node_q int64[nnodes]) from the per-edge 'Q'
        attribute with Q_default as fallback (_mjp_dense.py:355-356).
        Identical matrix objects share one slot."""
        slots = {}
        mats = []
        node_q = np.zeros(self.nnodes, dtype=np.int64)
        for i in range(1, self.nnodes):
            Q = self.edge_data[i].get('Q', Q_default)
            key = id(Q)
            if key not in slots:            # every distinct matrix is checked once
                check_square_dense(Q)
                if Q.shape[0] != nstates:
                    raise ValueError('rate matrix shape %s does not match nstates '
                                     '%d' % (Q.shape, nstates))
                slots[key] = len(mats)
                mats.append(np.ascontiguousarray(Q, dtype=np.float64))
            node_q[i] = slots[key]
        if not mats:
            mats.append(np.zeros((nstates, nstates)))
        return np.stack(mats), node_q

    def esd_transitions(self, nstates, P_default=None):
        """f64[nnodes,n,n] of the edges' 'P' (_density.py:143-180)."""
        esd = np.zeros((self.nnodes, nstates, nstates), dtype=np.float64)
        for i in range(1, self.nnodes):
            P = self.edge_data[i].get('P', P_default)
            check_square_dense(P)
            esd[i] = P
        return esd


def marshal_tree(T, root):
    return TreeArrays(T, root)


def nni_apply(T, root, v, c, s):
    """The tree after the nearest-neighbour interchange (v, c, s) of rt_model_nni_moves, on node
    LABELS of the networkx tree T rooted at `root`: c a child of v, s a sibling of v; the
    subtrees of c and s change places, and every edge's attributes follow the node below the
    edge (the data of v-c becomes that of p-c, p = parent(v); that of p-s becomes that of v-s).
    A new graph of T's class with T's node and graph attributes; s takes the place of c among
    the children of v and c that of s among the children of p, every other child order stays
    (so the preorder indices of the untouched nodes before v do, too).  ValueError for a triple
    that is not a move."""
    ta = TreeArrays(T, root)
    idx = ta.node_to_index
    if v not in idx or c not in idx or s not in idx:
        raise ValueError('(%r, %r, %r): not nodes of the tree' % (v, c, s))
    iv, ic, is_ = idx[v], idx[c], idx[s]
    if iv == 0:
        raise ValueError('%r is the root: no edge above it to move about' % (v,))
    ip = int(ta.parent[iv])
    if ta.parent[ic] != iv:
        raise ValueError('%r is not a child of %r' % (c, v))
    if is_ == iv or ta.parent[is_] != ip:
        raise ValueError('%r is not a sibling of %r' % (s, v))
    swap = {(iv, ic): is_, (ip, is_): ic}
    out = T.__class__()
    out.graph.update(T.graph)
    out.add_nodes_from((x, dict(T.nodes[x])) for x in ta.preorder_nodes)
    stack = [0]
    while stack:
        a = stack.pop()
        kids = [swap.get((a, int(b)), int(b)) for b in ta.indices[ta.indptr[a]:ta.indptr[a + 1]]]
        for b in kids:
            out.add_edge(ta.preorder_nodes[a], ta.preorder_nodes[b], **dict(ta.edge_data[b]))
        stack.extend(reversed(kids))
    return out


def place_apply(T, root, v, fraction, pendant, label, cut_label=None):
    """The tree with a query placed at (v, fraction, pendant) of rt_sites_placements, on node
    LABELS of the networkx tree T rooted at `root`: a new node `cut_label` (default
    ('cut', label)) cuts the edge p-v, p = parent(v), at `fraction` of its length from p, and
    the new leaf `label` hangs below it on an edge of length `pendant`.  A new graph of T's
    class with T's node and graph attributes; the cut node takes the place of v among the
    children of p, v is its first child and the new leaf its second.  Every attribute of the
    edge p-v is copied to the three edges (its rate matrix 'Q' among them), and 'weight', the
    length TreeArrays.branch_lengths reads, is set to fraction * t, (1 - fraction) * t and
    pendant.  ValueError for the root, an unknown node, a label already in the tree, or a
    fraction outside [0, 1]."""
    ta = TreeArrays(T, root)
    idx = ta.node_to_index
    if v not in idx:
        raise ValueError('%r is not a node of the tree' % (v,))
    iv = idx[v]
    if iv == 0:
        raise ValueError('%r is the root: no edge above it to place a query on' % (v,))
    if cut_label is None:
        cut_label = ('cut', label)
    if label in idx or cut_label in idx or label == cut_label:
        raise ValueError('the labels %r and %r must be new and distinct' % (label, cut_label))
    fraction, pendant = float(fraction), float(pendant)
    if not 0.0 <= fraction <= 1.0:
        raise ValueError('the fraction %r is outside [0, 1]' % (fraction,))
    if not (pendant >= 0.0 and pendant < float('inf')):
        raise ValueError('the pendant length %r is negative or not finite' % (pendant,))
    data = dict(ta.edge_data[iv])
    t = data.get('weight', 0.0)
    out = T.__class__()
    out.graph.update(T.graph)
    out.add_nodes_from((x, dict(T.nodes[x])) for x in ta.preorder_nodes)
    stack = [0]
    while stack:
        a = stack.pop()
        kids = [int(b) for b in ta.indices[ta.indptr[a]:ta.indptr[a + 1]]]
        for b in kids:
            if b != iv:
                out.add_edge(ta.preorder_nodes[a], ta.preorder_nodes[b], **dict(ta.edge_data[b]))
                continue
            out.add_edge(ta.preorder_nodes[a], cut_label, **dict(data, weight=fraction * t))
            out.add_edge(cut_label, v, **dict(data, weight=(1.0 - fraction) * t))
            out.add_edge(cut_label, label, **dict(data, weight=pendant))
        stack.extend(reversed(kids))
    return out


def spr_apply(T, root, c, y, fraction, cut_label=None):
    """The tree after the move (c, y) of rt_sites_spr_scores at `fraction`, on node LABELS of the
    networkx tree T rooted at `root`: the subtree of c leaves its parent and comes with every
    attribute of its edge; a new node `cut_label` (default ('cut', c)) cuts the edge q-y,
    q = parent(y), at `fraction` of its length from q, and c hangs below it.  A new graph of
    T's class with T's node and graph attributes; the cut node stands in the place of y among
    the children of q, y is its first child and c its second; the parent of c keeps its other
    children.  Every attribute of the edge q-y is copied to its two halves (its rate matrix
    'Q' among them), and 'weight', the length TreeArrays.branch_lengths reads, is set to
    fraction * t and (1 - fraction) * t, as place_apply splits an edge.  ValueError for an
    unknown node, the root as c or y, y inside the subtree of c, a label already in the tree,
    or a fraction outside [0, 1]."""
    ta = TreeArrays(T, root)
    idx = ta.node_to_index
    for x in (c, y):
        if x not in idx:
            raise ValueError('%r is not a node of the tree' % (x,))
    ic, iy = idx[c], idx[y]
    if ic == 0 or iy == 0:
        raise ValueError('the root is neither pruned nor below an edge to regraft on')
    a = iy
    while a >= 0:
        if a == ic:
            raise ValueError('%r lies in the subtree of %r' % (y, c))
        a = int(ta.parent[a])
    if cut_label is None:
        cut_label = ('cut', c)
    if cut_label in idx:
        raise ValueError('the label %r must be new' % (cut_label,))
    fraction = float(fraction)
    if not 0.0 <= fraction <= 1.0:
        raise ValueError('the fraction %r is outside [0, 1]' % (fraction,))
    data = dict(ta.edge_data[iy])
    t = data.get('weight', 0.0)
    out = T.__class__()
    out.graph.update(T.graph)
    out.add_nodes_from((x, dict(T.nodes[x])) for x in ta.preorder_nodes)
    stack = [0]
    while stack:
        a = stack.pop()
        kids = [int(b) for b in ta.indices[ta.indptr[a]:ta.indptr[a + 1]]]
        for b in kids:
            if b == ic:
                continue
            if b != iy:
                out.add_edge(ta.preorder_nodes[a], ta.preorder_nodes[b], **dict(ta.edge_data[b]))
                continue
            out.add_edge(ta.preorder_nodes[a], cut_label, **dict(data, weight=fraction * t))
            out.add_edge(cut_label, y, **dict(data, weight=(1.0 - fraction) * t))
            out.add_edge(cut_label, c, **dict(ta.edge_data[ic]))
        stack.extend(reversed(kids))
    return out
