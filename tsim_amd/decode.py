"""A maximum-likelihood lookup-table decoder, built from pattern counts and applied where the shots are.

``train = sampler.count(N, pattern_columns="all")`` returns which (detectors, observables) patterns occurred and how
often; :meth:`LookupDecoder.from_counts` keeps, per detector pattern (syndrome), the observable pattern seen most often.
``sampler.count(M, decoder=dec)`` then looks every kept shot's syndrome up on the GPU (a row table loaded from the host,
``tsim_rowtab_load`` / ``tsim_rowtab_decode_device``, ``csrc/tsim_rowtab.hip.h``) and counts the shots whose observables
differ from the prediction (``ShotCounts.decoded_errors``) and those whose syndrome is unknown
(``ShotCounts.decoder_misses``); :meth:`LookupDecoder.decode` / :meth:`LookupDecoder.missed` are the same in numpy.

A union-find (cluster-growth) decoder over the decoding graph of a Clifford circuit
------------------------------------------------------------------------------------
A table of syndromes stops at d = 3 .. 5: beyond that almost every syndrome is new.  :class:`UnionFindDecoder` needs no
training run: it decodes on the graph of the circuit's error bits and always returns a correction that reproduces the
syndrome (or reports a miss).  ``sampler.count(M, decoder=uf)`` runs it on the GPU (``tsim_uf_*``, ``csrc/tsim_uf.hip.h``);
:meth:`UnionFindDecoder.decode` / :meth:`UnionFindDecoder.missed` are the numpy statement and the oracle of the GPU tests.

The graph (:class:`DecodingGraph`, from the ``FaultForm`` of ``CliffordCircuit.compile_faults()``).  Node 0 is the boundary,
node ``i + 1`` is detector ``i``.  The marginal of an error bit is the sum of its site's outcome probabilities over the
outcomes that have the bit set; bits of marginal 0 are skipped.  A bit that flips the detector nodes ``{a}`` gives the pair
``(0, a)``, one that flips ``{a, b}``, ``a < b``, gives ``(a, b)``; its observable mask is a uint64, bit ``k`` = observable
``k``.  Bits of one pair merge: within one mask the probabilities combine as ``p (1 - q) + q (1 - p)`` (in the order of the
bits); of several masks the one with the largest combined probability is kept, a tie going to the smaller mask.  Edges are
numbered in ascending ``(u, v)`` order.  A bit without a detector and with an observable counts in ``undetectable_bits``, a
bit with more than two detectors in ``dropped_bits`` (:meth:`DecodingGraph.info`); neither is refused.  At most 65535
nodes and 65535 edges (uint16 indices on the device).  ``edge_p`` gives the edge caps of weighted growth (below); without
caps the decoder is UNWEIGHTED.

The decoding rule, stated so that no parallel order can change the answer.  For one shot ``defect[v]`` is the bit of
detector ``v - 1``, ``defect[0] = 0``; every edge has an integer cap ``cap[e]`` in 1 .. 14 (2 everywhere when the decoder
is unweighted) and ``grown[e]`` in ``0 .. cap[e]``, 0 at first; an edge is FULL when ``grown[e] == cap[e]``.

1. Growth, in synchronous rounds.  Clusters are the connected components of the nodes under the full edges
   (every node is at least its own cluster).  A cluster is ACTIVE when it holds an odd number of defects and does not
   contain node 0.  No active cluster: growth ends.  Otherwise, from the state at the start of the round, every edge gets
   ``grown[e] = min(cap[e], grown[e] + active(cluster(u)) + active(cluster(v)))``.  A round that changes nothing while a cluster
   is active makes the shot a MISS (no flip is predicted): it happens only in a component without a boundary edge.
2. Forest.  The root of a cluster is its node of smallest index (node 0 whenever the cluster contains it); ``level(v)`` is
   the distance from the root over full edges; the parent edge of ``v`` is the smallest-index such edge to a node
   of ``level(v) - 1``.
3. Peeling, from the deepest level up.  ``s = defect``; a node ``v`` that is not a root and has ``s[v] = 1`` flips its
   parent edge ``e``: both ends of ``e`` toggle in ``s`` and ``prediction ^= edge_obs[e]``.  Afterwards ``s`` is zero off
   node 0 (asserted in the numpy statement).

Weighted growth.  A likely edge should fill sooner than an unlikely one: :meth:`DecodingGraph.growth_caps` turns ``edge_p``
into caps, in float64: ``q = clip(edge_p, 1e-12, 0.5)``, ``L = log((1 - q) / q)``,
``cap = clip(rint(2 * resolution * L / L.max()), 1, 2 * resolution)`` (``2 * resolution`` everywhere when ``L.max() == 0``), so
the least likely edge gets ``2 * resolution`` and the likeliest edges the smallest caps.  ``resolution`` is 1 .. 7 (caps stop
at 14: the device counts ``grown`` in 4 bits and may pass the cap by one).  The default is 4.  Resolution 1 quantises to the
caps {1, 2} and is WORSE than no weights (110 decoded errors against 12 at d = 3, p = 1e-3); a higher
resolution costs growth rounds in proportion.  ``UnionFindDecoder.from_circuit(circuit, weights="probability")`` uses these
caps; ``weights=None`` (caps of 2 everywhere, bit for bit) stays the default.

Heralded erasures (``DecodingGraph.from_form(form, heralds=True)``, ``UnionFindDecoder.from_circuit(circuit, heralds=True)``;
``heralds=False`` is the default and leaves every array, number and prediction what it is above).  A herald tells where an
error may be, so the edges of the heralded site start fully grown and the herald itself is no syndrome bit.

Herald bits are found from the ``FaultForm`` alone.  Within a site of ``k >= 2`` error bits with outcome table ``P``, bit ``i``
is a HERALD BIT iff (a) every outcome ``o != 0`` with ``P[o] > 0`` has bit ``i`` set, and there is such an outcome; (b) its
column list is exactly one output, a detector ``h < num_detectors`` with ``out_const[h] == 0``; (c) no other error bit of the
circuit lists ``h``.  Then ``h`` is a HERALD DETECTOR: it is 1 exactly when the site fired.  Of several such bits of a site the
lowest is the herald, the others are ordinary bits.  A detector that fails (c) - one that XORs two herald records, say -
stays an ordinary detector.

The graph with heralds.  Herald detectors are not nodes: node 0 is the boundary, node ``v >= 1`` is the ``v``-th non-herald
detector in column order, ``node_det[v - 1]`` is its column (``arange`` without heralds) and ``num_detectors`` is the number of
detector columns of a row, ``n_nodes - 1 + n_heralds``.  Herald bits give no edge; every other bit contributes as above, in
the new node numbers, the non-herald bits of heralded sites included, with their unconditional marginals.  Per herald, in
herald-column order, a CSR (``herald_det``, ``herald_ptr``, ``herald_edges``) lists the distinct edges, ascending, of the site's
other bits that have marginal > 0 and flip one or two non-herald detectors; such bits with more than two detectors count in
``info()["herald_bits_dropped"]``, bits without a detector are ignored, and a herald's list may be empty.

The rule with heralds changes at its start only.  ``defect[v]`` is the bit of column ``node_det[v - 1]``; for every herald
whose column is set, every listed edge starts at ``grown[e] = cap[e]``.  Growth, forest and peeling are as written (the
clusters of the pre-grown edges exist in round 1).  A row whose non-herald detectors are all 0 predicts 0 and is not
decoded, whatever its heralds say.
"""

from __future__ import annotations

import numpy as np

__all__ = ["LookupDecoder", "DecodingGraph", "UnionFindDecoder"]

MAX_GRAPH = 65535  # nodes, and edges: uint16 indices on the device
MAX_CAP = 14       # of an edge: the device counts grown[e] in 4 bits and may pass the cap by one


def _pack(bits: np.ndarray) -> np.ndarray:
    return np.packbits(np.asarray(bits, dtype=np.bool_), axis=1, bitorder="little")


def _as_uint64(bits: np.ndarray) -> np.ndarray:
    """bool ``[n, k]`` (``k <= 64``) -> uint64 ``[n]``, bit ``i`` = column ``i``."""
    out = np.zeros((len(bits), 8), dtype=np.uint8)
    p = _pack(bits)
    out[:, : p.shape[1]] = p
    return out.view("<u8").reshape(len(bits))


class LookupDecoder:
    """``syndromes`` bool ``[D, num_detectors]`` (distinct rows) with ``predictions`` bool ``[D, num_observables]``
    (at most 64 observables): a shot with syndrome ``syndromes[i]`` is predicted to have flipped ``predictions[i]``; a
    syndrome that is not listed predicts no flip."""

    def __init__(self, syndromes, predictions):
        s = np.asarray(syndromes, dtype=np.bool_)
        p = np.asarray(predictions, dtype=np.bool_)
        if s.ndim != 2 or p.ndim != 2 or len(s) != len(p):
            raise ValueError(f"syndromes [D, nd] and predictions [D, n_obs] expected, got shapes {s.shape} and {p.shape}")
        if p.shape[1] > 64:
            raise ValueError(f"at most 64 observables, got {p.shape[1]}")
        self.syndromes, self.predictions = s.copy(), p.copy()
        self._keys = _pack(s).reshape(len(s), (s.shape[1] + 7) // 8)
        self._index = {k.tobytes(): i for i, k in enumerate(self._keys)}
        if len(self._index) != len(s):
            raise ValueError("the syndromes must be distinct")

    @property
    def num_detectors(self) -> int:
        return self.syndromes.shape[1]

    @property
    def num_observables(self) -> int:
        return self.predictions.shape[1]

    def __len__(self) -> int:
        return len(self.syndromes)

    def table(self):
        """``(keys uint8[D, ceil(nd/8)], values uint64[D])``: the bit-packed syndromes and predictions (bit ``i`` = observable
        ``i``), as ``tsim_rowtab_load`` takes them."""
        return self._keys, _as_uint64(self.predictions)

    @classmethod
    def from_counts(cls, counts) -> "LookupDecoder":
        """From a ``ShotCounts`` whose ``pattern_columns`` are all the detectors followed by all the observables
        (``count(N, pattern_columns="all")``): per syndrome the observable pattern with the largest count, a tie going to
        the smaller packed value (bit ``i`` = observable ``i``)."""
        n_cols, nd = len(counts.column_counts), int(counts.num_detectors)
        if counts.patterns is None or tuple(counts.pattern_columns) != tuple(range(n_cols)):
            raise ValueError('the counts must carry the patterns over every column: count(..., pattern_columns="all")')
        if n_cols - nd > 64:
            raise ValueError(f"at most 64 observables, got {n_cols - nd}")
        pat, cnt = np.asarray(counts.patterns, dtype=np.bool_), np.asarray(counts.pattern_counts, dtype=np.int64)
        if len(pat) == 0:
            return cls(np.zeros((0, nd), np.bool_), np.zeros((0, n_cols - nd), np.bool_))
        uniq, inv = np.unique(_pack(pat[:, :nd]).reshape(len(pat), (nd + 7) // 8), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        val = _as_uint64(pat[:, nd:])
        order = np.lexsort((val, -cnt, inv))  # per syndrome: the largest count first, then the smaller value
        first = order[np.concatenate([[True], inv[order][1:] != inv[order][:-1]])]
        return cls(pat[first, :nd], pat[first, nd:])

    def _lookup(self, dets) -> np.ndarray:
        """The entry of each row's syndrome, -1 for an unknown one."""
        d = np.asarray(dets, dtype=np.bool_)
        if d.ndim != 2 or d.shape[1] != self.num_detectors:
            raise ValueError(f"dets must be [n, {self.num_detectors}], got shape {d.shape}")
        if len(d) == 0:
            return np.zeros(0, dtype=np.int64)
        uniq, inv = np.unique(_pack(d).reshape(len(d), (d.shape[1] + 7) // 8), axis=0, return_inverse=True)
        idx = np.fromiter((self._index.get(k.tobytes(), -1) for k in uniq), np.int64, len(uniq))
        return idx[np.asarray(inv).reshape(-1)]

    def decode(self, dets) -> np.ndarray:
        """bool ``[n, num_observables]``: the predicted observable flips of detector rows bool ``[n, num_detectors]``."""
        idx = self._lookup(dets)
        out = np.zeros((len(idx), self.num_observables), dtype=np.bool_)
        out[idx >= 0] = self.predictions[idx[idx >= 0]]
        return out

    def missed(self, dets) -> np.ndarray:
        """bool ``[n]``: the rows whose syndrome is not in the table."""
        return self._lookup(dets) < 0


class DecodingGraph:
    """The decoding graph (module docstring): ``n_nodes`` (node 0 the boundary), ``edge_u < edge_v`` (int32, strictly
    ascending pairs), ``edge_obs`` (uint64 observable masks) and ``edge_p`` (float64; :meth:`growth_caps` makes edge caps of it)."""

    def __init__(self, n_nodes: int, edge_u, edge_v, edge_obs, edge_p=None, *, dropped_bits: int = 0, undetectable_bits: int = 0,
                 node_det=None, herald_det=None, herald_ptr=None, herald_edges=None, herald_bits_dropped: int = 0):
        u, v = np.asarray(edge_u), np.asarray(edge_v)
        if u.ndim != 1 or v.shape != u.shape or np.asarray(edge_obs).shape != u.shape:
            raise ValueError(f"edge_u, edge_v and edge_obs must be 1-D and equally long, got shapes {u.shape}, {v.shape} and "
                             f"{np.asarray(edge_obs).shape}")
        if int(n_nodes) != n_nodes or n_nodes < 2:
            raise ValueError(f"n_nodes = {n_nodes!r}: the boundary and at least one detector")
        if n_nodes > MAX_GRAPH or len(u) > MAX_GRAPH:
            raise NotImplementedError(f"{n_nodes} nodes and {len(u)} edges (at most {MAX_GRAPH} each: indices are uint16 on the device)")
        if len(u) and not (np.issubdtype(u.dtype, np.integer) and np.issubdtype(v.dtype, np.integer)):
            raise ValueError("edge_u and edge_v must be integers")
        u, v = u.astype(np.int64), v.astype(np.int64)
        if len(u) and (u.min() < 0 or v.max() >= n_nodes or v.min() < 0 or u.max() >= n_nodes):
            raise ValueError(f"edge ends must lie in 0 .. {int(n_nodes) - 1}")
        if (u >= v).any():
            raise ValueError(f"edge {int(np.flatnonzero(u >= v)[0])}: u < v expected")
        key = u * int(n_nodes) + v
        if (np.diff(key) <= 0).any():
            raise ValueError(f"edge {int(np.flatnonzero(np.diff(key) <= 0)[0]) + 1}: the pairs (u, v) must be strictly ascending")
        p = np.zeros(len(u)) if edge_p is None else np.asarray(edge_p, dtype=np.float64)
        if p.shape != u.shape:
            raise ValueError(f"edge_p must have shape {u.shape}, got {p.shape}")
        self.n_nodes = int(n_nodes)
        self.edge_u, self.edge_v = u.astype(np.int32), v.astype(np.int32)
        self.edge_obs = np.asarray(edge_obs).astype(np.uint64)
        self.edge_p = p.copy()
        self.dropped_bits, self.undetectable_bits = int(dropped_bits), int(undetectable_bits)
        self._set_heralds(node_det, herald_det, herald_ptr, herald_edges)
        self.herald_bits_dropped = int(herald_bits_dropped)

    def _set_heralds(self, node_det, herald_det, herald_ptr, herald_edges):
        """The columns of the nodes and the heralds' CSR (module docstring), checked; without them every column is a node."""
        def ints(name, a, n=None):
            a = np.zeros(0, np.int64) if a is None else np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)) or (n is not None and a.size != n):
                raise ValueError(f"{name} must be 1-D integers" + ("" if n is None else f", {n} of them"))
            if a.size and (a.min() < 0 or a.max() > 0x7FFFFFFF):
                raise ValueError(f"{name} must lie in 0 .. 2^31 - 1")
            return a.astype(np.int64)

        hd = ints("herald_det", herald_det)
        nh = len(hd)
        nd = self.n_nodes - 1 + nh
        if nd > 0x7FFFFFFF:
            raise ValueError(f"{nd} detector columns (at most 2^31 - 1)")
        nodes = np.arange(self.n_nodes - 1, dtype=np.int64) if node_det is None else ints("node_det", node_det, self.n_nodes - 1)
        hp = np.zeros(1, np.int64) if herald_ptr is None and nh == 0 else ints("herald_ptr", herald_ptr, nh + 1)
        he = ints("herald_edges", herald_edges)
        if (np.diff(nodes) <= 0).any():
            raise ValueError(f"node_det[{int(np.flatnonzero(np.diff(nodes) <= 0)[0]) + 1}]: the columns of the nodes must be strictly ascending")
        cols = np.concatenate([nodes, hd])
        if len(cols) and cols.max() >= nd:
            raise ValueError(f"column {int(cols.max())} of {nd} detector columns ({self.n_nodes - 1} nodes and {nh} heralds)")
        seen = np.bincount(cols, minlength=nd)
        if (seen > 1).any():
            raise ValueError(f"column {int(np.flatnonzero(seen > 1)[0])} is named twice (a column is a node or one herald)")
        if hp[0] != 0 or (np.diff(hp) < 0).any() or hp[-1] != len(he):
            raise ValueError(f"herald_ptr must rise from 0 to len(herald_edges) = {len(he)}")
        if len(he) and he.max() >= self.n_edges:
            raise ValueError(f"herald_edges names edge {int(he.max())} of {self.n_edges}")
        self.node_det, self.herald_det = nodes.astype(np.int32), hd.astype(np.int32)
        self.herald_ptr, self.herald_edges = hp.astype(np.int32), he.astype(np.int32)

    @property
    def n_edges(self) -> int:
        return len(self.edge_u)

    @property
    def n_heralds(self) -> int:
        return len(self.herald_det)

    @property
    def num_detectors(self) -> int:
        """The detector columns of a row: the nodes but the boundary, and the heralds."""
        return self.n_nodes - 1 + self.n_heralds

    def info(self) -> dict:
        deg = np.bincount(np.concatenate([self.edge_u, self.edge_v]), minlength=self.n_nodes)
        return dict(n_nodes=self.n_nodes, n_edges=self.n_edges, dropped_bits=self.dropped_bits,
                    undetectable_bits=self.undetectable_bits, boundary_degree=int(deg[0]),
                    max_node_degree=int(deg[1:].max()) if self.n_nodes > 1 else 0, n_heralds=self.n_heralds,
                    herald_bits_dropped=self.herald_bits_dropped)

    def growth_caps(self, resolution: int = 4) -> np.ndarray:
        """``uint8[n_edges]``: the caps of weighted growth from ``edge_p`` (module docstring), 1 .. ``2 * resolution``;
        ``resolution`` is an int in 1 .. 7."""
        if isinstance(resolution, (bool, np.bool_)) or not isinstance(resolution, (int, np.integer)) or not 1 <= resolution <= MAX_CAP // 2:
            raise ValueError(f"resolution = {resolution!r}: an int in 1 .. {MAX_CAP // 2}")
        top = 2 * int(resolution)
        if not self.n_edges:
            return np.zeros(0, np.uint8)
        q = np.clip(self.edge_p.astype(np.float64), 1e-12, 0.5)
        L = np.log((1.0 - q) / q)
        if L.max() == 0:
            return np.full(self.n_edges, top, np.uint8)
        return np.clip(np.rint(top * L / L.max()), 1, top).astype(np.uint8)

    @staticmethod
    def _herald_bits(form) -> dict:
        """``{error bit: herald detector column}`` by the criterion of the module docstring."""
        nd = int(form.num_detectors)
        listed = np.bincount(np.asarray(form.cols, dtype=np.int64), minlength=int(form.n_out))
        out, e0 = {}, 0
        for probs in form.channel_probs:
            probs = np.asarray(probs, dtype=np.float64)
            k = int(len(probs)).bit_length() - 1
            fired = np.flatnonzero(probs > 0)
            fired = fired[fired != 0]
            if k >= 2 and len(fired):
                for i in range(k):
                    if not ((fired >> i) & 1).all():
                        continue
                    cols = form.cols[form.col_ptr[e0 + i]:form.col_ptr[e0 + i + 1]]
                    if len(cols) == 1 and cols[0] < nd and form.out_const[cols[0]] == 0 and listed[cols[0]] == 1:
                        out[e0 + i] = int(cols[0])
                        break  # (the lowest such bit is the herald, the others are ordinary bits)
            e0 += k
        return out

    @classmethod
    def from_form(cls, form, heralds: bool = False) -> "DecodingGraph":
        """From the ``FaultForm`` of ``CliffordCircuit.compile_faults()`` (module docstring).  ``heralds``: herald detectors
        are not nodes, their sites' edges are listed per herald."""
        if getattr(form, "kind", None) != "detectors":
            raise ValueError("the decoding graph needs the form of compile_faults()")
        nd, n_obs = int(form.num_detectors), int(form.n_out) - int(form.num_detectors)
        if n_obs > 64:
            raise ValueError(f"at most 64 observables, got {n_obs}")
        if nd < 1:
            raise ValueError("a decoder needs at least one detector")
        herald_of = cls._herald_bits(form) if heralds else {}
        herald_cols = np.array(sorted(herald_of.values()), np.int64)
        node_det = np.setdiff1d(np.arange(nd), herald_cols)
        if len(node_det) < 1:
            raise ValueError("a decoder needs at least one detector that is not a herald")
        if len(node_det) + 1 > MAX_GRAPH:
            raise NotImplementedError(f"{len(node_det) + 1} nodes (at most {MAX_GRAPH}: indices are uint16 on the device)")
        node_of = np.full(nd, -1, np.int64)   # detector column -> node
        node_of[node_det] = np.arange(1, len(node_det) + 1)
        pairs: dict = {}   # (u, v) -> {mask: probability}
        site_pairs: dict = {}   # herald column -> the pairs of its site's other bits
        dropped = undetectable = herald_dropped = 0
        e0 = 0
        for probs in form.channel_probs:
            probs = np.asarray(probs, dtype=np.float64)
            k = int(len(probs)).bit_length() - 1
            outcomes = np.arange(len(probs))
            site_herald = next((herald_of[e0 + i] for i in range(k) if e0 + i in herald_of), None)
            if site_herald is not None:
                site_pairs[site_herald] = set()
            for i in range(k):
                e = e0 + i
                if e in herald_of:
                    continue
                p = float(probs[((outcomes >> i) & 1).astype(np.bool_)].sum())
                if p <= 0.0:
                    continue
                cols = form.cols[form.col_ptr[e]:form.col_ptr[e + 1]]
                dets = sorted(int(node_of[c]) for c in cols if c < nd)
                mask = 0
                for c in cols:
                    if c >= nd:
                        mask |= 1 << (int(c) - nd)
                if not dets:
                    undetectable += bool(mask)
                    continue
                if len(dets) > 2:
                    dropped += 1
                    herald_dropped += site_herald is not None
                    continue
                pair = (0, dets[0]) if len(dets) == 1 else (dets[0], dets[1])
                if site_herald is not None:
                    site_pairs[site_herald].add(pair)
                by_mask = pairs.setdefault(pair, {})
                q = by_mask.get(mask, 0.0)
                by_mask[mask] = p * (1.0 - q) + q * (1.0 - p)
            e0 += k
        if len(pairs) > MAX_GRAPH:
            raise NotImplementedError(f"{len(pairs)} edges (at most {MAX_GRAPH}: indices are uint16 on the device)")
        order = sorted(pairs)
        best = [min(pairs[pr].items(), key=lambda mp: (-mp[1], mp[0])) for pr in order]   # the likelier mask, a tie to the smaller
        extra = {}
        if heralds:
            index = {pr: e for e, pr in enumerate(order)}
            lists = [sorted(index[pr] for pr in site_pairs[h]) for h in herald_cols.tolist()]
            extra = dict(node_det=node_det, herald_det=herald_cols, herald_ptr=np.cumsum([0] + [len(x) for x in lists]),
                         herald_edges=np.array([e for x in lists for e in x], np.int64), herald_bits_dropped=herald_dropped)
        return cls(len(node_det) + 1, np.array([pr[0] for pr in order], np.int32), np.array([pr[1] for pr in order], np.int32),
                   np.array([m for m, _ in best], np.uint64), np.array([p for _, p in best], np.float64),
                   dropped_bits=dropped, undetectable_bits=undetectable, **extra)


def uf_shot_bytes(n_nodes: int, n_edges: int, weighted: bool) -> int:
    """The LDS bytes of one shot's state on the device (``layout()`` of ``csrc/tsim_uf.hip.h``): per node a uint16 label, a
    uint32 level and parent edge and two bytes; per 32 edges the ``full`` bitmap word and its uint16 list entry, and either
    the ``half`` bitmap word or, under weighted growth, four words of 4-bit counters; 16 bytes of scalars."""
    a16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    w32 = max(1, (n_edges + 31) // 32)
    grown = max(1, (n_edges + 7) // 8) if weighted else w32
    return a16(2 * n_nodes) + a16(4 * n_nodes) + 2 * a16(n_nodes) + a16(4 * grown) + a16(4 * w32) + a16(2 * w32) + 16


def _components(label: np.ndarray, fu: np.ndarray, fv: np.ndarray) -> np.ndarray:
    """Min-label propagation over the edges ``(fu, fv)``, from labels that are upper bounds (each a node of its own cluster),
    to its fixpoint."""
    while len(fu):
        m = np.minimum(label[fu], label[fv])
        if (m == label[fu]).all() and (m == label[fv]).all():
            break
        np.minimum.at(label, fu, m)
        np.minimum.at(label, fv, m)
        label = label[label]  # (a label is a node of the same cluster, label[x] <= x: the fixpoint is the same, in fewer sweeps)
    return label


class UnionFindDecoder:
    """The union-find decoder of a :class:`DecodingGraph` (module docstring) for rows of ``graph.num_detectors`` detectors and
    ``num_observables`` observables (default: as many as the masks of the graph use, at least one; at most 64).
    ``decode`` / ``missed`` have the signatures of :class:`LookupDecoder`; they decode each distinct syndrome once.
    ``edge_caps``: an integer per edge in 1 .. 14 for weighted growth (kept as uint8 in ``self.edge_caps``), ``None`` for the
    unweighted decoder (a cap of 2 everywhere)."""

    def __init__(self, graph: DecodingGraph, num_observables: int | None = None, edge_caps=None):
        used = int(np.bitwise_or.reduce(graph.edge_obs)) if graph.n_edges else 0
        n_obs = max(1, used.bit_length()) if num_observables is None else int(num_observables)
        if n_obs > 64:
            raise ValueError(f"at most 64 observables, got {n_obs}")
        if used >> n_obs:
            raise ValueError(f"an edge flips observable {used.bit_length() - 1}, the rows have {n_obs}")
        if edge_caps is not None:
            caps = np.asarray(edge_caps)
            if caps.shape != (graph.n_edges,):
                raise ValueError(f"edge_caps must have shape ({graph.n_edges},), got {caps.shape}")
            if not np.issubdtype(caps.dtype, np.integer):
                raise ValueError(f"edge_caps must be integers, got {caps.dtype}")
            if len(caps) and (caps.min() < 1 or caps.max() > MAX_CAP):
                bad = int(np.flatnonzero((caps < 1) | (caps > MAX_CAP))[0])
                raise ValueError(f"edge {bad} has cap {int(caps[bad])} (1 .. {MAX_CAP})")
            edge_caps = caps.astype(np.uint8)
        self.graph, self._n_obs, self.edge_caps = graph, n_obs, edge_caps
        self._cache: dict = {}   # packed row of detectors -> (prediction, missed, flipped edges, rounds)

    @classmethod
    def from_circuit(cls, circuit, weights: str | None = None, resolution: int = 4, heralds: bool = False) -> "UnionFindDecoder":
        """Of a :class:`tsim_amd.clifford.CliffordCircuit` with deterministic detectors (or its program text).  ``weights``:
        ``None`` (unweighted) or ``"probability"``: the caps ``graph.growth_caps(resolution)`` (module docstring).
        ``heralds``: herald detectors pre-grow their site's edges and are no syndrome bits (module docstring)."""
        if weights not in (None, "probability"):
            raise ValueError(f'weights = {weights!r}: None or "probability"')
        if isinstance(circuit, str):
            from .clifford import CliffordCircuit

            circuit = CliffordCircuit(circuit)
        form = circuit.compile_faults()
        graph = DecodingGraph.from_form(form, heralds=heralds)
        return cls(graph, int(form.n_out) - int(form.num_detectors), None if weights is None else graph.growth_caps(resolution))

    @property
    def num_detectors(self) -> int:
        return self.graph.num_detectors

    @property
    def num_observables(self) -> int:
        return self._n_obs

    def info(self) -> dict:
        return self.graph.info()

    # -- the numpy statement ---------------------------------------------------------------------------------------------
    def _decode_one(self, defects: np.ndarray, erased_edges=()):
        """One syndrome (the defect NODES, ascending; ``erased_edges`` start fully grown): ``(prediction, missed, flipped edges
        ascending, growth rounds)``."""
        g = self.graph
        n, eu, ev = g.n_nodes, g.edge_u, g.edge_v
        defect = np.zeros(n, np.bool_)
        defect[defects] = True
        cap = np.full(g.n_edges, 2, np.int8) if self.edge_caps is None else self.edge_caps.astype(np.int8)
        grown = np.zeros(g.n_edges, np.int8)
        erased = np.asarray(erased_edges, dtype=np.int64)
        grown[erased] = cap[erased]
        label = np.arange(n)
        rounds = 0
        while True:
            f = grown == cap
            label = _components(label, eu[f], ev[f])
            odd = (np.bincount(label[defect], minlength=n) & 1).astype(np.bool_)
            odd[0] = False
            active = odd[label]
            if not active.any():
                break
            new = np.minimum(cap, grown + active[eu] + active[ev]).astype(np.int8)
            if np.array_equal(new, grown):
                return 0, True, np.zeros(0, np.int64), rounds
            grown, rounds = new, rounds + 1
        # the forest: levels from the roots, the parent edge the smallest-index edge to the level above
        fe = np.flatnonzero(grown == cap)
        fu, fv = eu[fe], ev[fe]
        level = np.where(label == np.arange(n), 0, -1)
        parent = np.full(n, -1, np.int64)
        depth = 0
        while True:
            down = (level[fu] == depth) & (level[fv] < 0)
            up = (level[fv] == depth) & (level[fu] < 0)
            child = np.concatenate([fv[down], fu[up]])
            if not len(child):
                break
            via = np.concatenate([fe[down], fe[up]])
            parent[child] = g.n_edges
            np.minimum.at(parent, child, via)
            level[child] = depth + 1
            depth += 1
        # peeling, from the deepest level up
        s = defect.copy()
        prediction, flipped = 0, []
        for lv in range(depth, 0, -1):
            for v in np.flatnonzero((level == lv) & s):
                e = int(parent[v])
                s[eu[e]] ^= True
                s[ev[e]] ^= True
                prediction ^= int(g.edge_obs[e])
                flipped.append(e)
        assert not s[1:].any(), "the correction does not reproduce the syndrome"
        return prediction, False, np.array(sorted(flipped), np.int64), rounds

    def _decoded(self, dets):
        """Per row the cache entry of its detector columns (``None`` for a row without defects, whatever its heralds)."""
        d = np.asarray(dets, dtype=np.bool_)
        if d.ndim != 2 or d.shape[1] != self.num_detectors:
            raise ValueError(f"dets must be [n, {self.num_detectors}], got shape {d.shape}")
        g = self.graph
        out = [None] * len(d)
        rows = np.flatnonzero(d[:, g.node_det].any(axis=1))
        if not len(rows):
            return out
        uniq, inv = np.unique(_pack(d[rows]), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        entries = []
        for k in uniq:
            key = k.tobytes()
            if key not in self._cache:
                bits = np.unpackbits(k, bitorder="little", count=self.num_detectors)
                erased = [g.herald_edges[g.herald_ptr[h]:g.herald_ptr[h + 1]] for h in np.flatnonzero(bits[g.herald_det])]
                self._cache[key] = self._decode_one(np.flatnonzero(bits[g.node_det]) + 1,
                                                    np.unique(np.concatenate(erased)) if erased else ())
            entries.append(self._cache[key])
        for r, i in zip(rows, inv):
            out[r] = entries[i]
        return out

    def predictions(self, dets) -> np.ndarray:
        """uint64 ``[n]``: the predicted observable mask of every row (bit ``k`` = observable ``k``; 0 for a miss) - what the
        device kernel writes to ``d_pred``."""
        return np.array([0 if e is None else e[0] for e in self._decoded(dets)], dtype=np.uint64)

    def decode(self, dets) -> np.ndarray:
        """bool ``[n, num_observables]``: the predicted observable flips of detector rows bool ``[n, num_detectors]``."""
        p = self.predictions(dets)
        return ((p[:, None] >> np.arange(self._n_obs, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.bool_)

    def missed(self, dets) -> np.ndarray:
        """bool ``[n]``: the rows whose growth stopped with an active cluster left (no flip is predicted for them)."""
        return np.array([e is not None and e[1] for e in self._decoded(dets)], dtype=np.bool_)

    def flipped_edges(self, dets) -> list:
        """Per row the edges of its correction (int64, ascending; empty for a row without defects and for a miss)."""
        return [np.zeros(0, np.int64) if e is None else e[2] for e in self._decoded(dets)]

    def growth_rounds(self, dets) -> np.ndarray:
        """int64 ``[n]``: the growth rounds every row took."""
        return np.array([0 if e is None else e[3] for e in self._decoded(dets)], dtype=np.int64)

    # -- the device side -------------------------------------------------------------------------------------------------
    def decode_device(self, hp, d_rows: int, n: int, row_bytes: int, *, n_cols: int | None = None, d_xor: int = 0, d_test: int = 0,
                      stream: int = 0):
        """``(predictions uint64[n], (kept, wrong, missed))`` for ``n`` bit-packed rows already in HBM (detectors, then
        observables; ``n_cols`` columns, default ``num_detectors + num_observables``; ``d_xor`` / ``d_test``: device masks of
        ``ceil(n_cols / 8)`` bytes) by one ``tsim_uf`` handle on ``hp``'s device, created and destroyed here.  A row that is
        not kept and a miss predict 0.  Returns when the results are on the host."""
        nd = self.num_detectors
        n_cols = nd + self._n_obs if n_cols is None else int(n_cols)
        h = hp.uf_create(self.graph, n_cols, self.edge_caps)
        bufs = []
        try:
            pred = np.zeros(int(n), np.uint64)
            cnt = np.zeros(3, np.uint64)
            d_pred, d_cnt = hp.malloc(pred.nbytes + 16), hp.malloc(cnt.nbytes + 16)
            bufs += [d_pred, d_cnt]
            hp.h2d(d_cnt, cnt)
            hp.uf_decode_device(h, d_rows, n, row_bytes, (nd, nd + self._n_obs), d_cnt.ptr, d_pred=d_pred.ptr, d_xor=d_xor,
                                d_test=d_test, stream=stream)
            hp.stream_synchronize(stream)
            if n:
                hp.d2h(pred, d_pred)
            hp.d2h(cnt, d_cnt)
            return pred, tuple(int(x) for x in cnt)
        finally:
            hp.uf_destroy(h)
            for b in bufs:
                b.free()
