"""The large inputs of the union-find decoder's GPU tests (``test_gpu_unionfind_large.py``), and the proof, from the numpy
statement alone, that they reach the code the small graphs never did: more than 64 listed words of the ``full`` bitmap
(the stride of ``full_edges()``), edge indices beyond 32767 (uint16 ``adj_edge`` / ``wlist``, the low half of ``lp``),
hundreds of levels, a miss next to hundreds of decoded clusters, a shot whose state fills a block's LDS to the last 16 bytes,
and every number of waves a block can have.  Every builder is seeded; the decoders cache the syndromes they have seen, so a
case is built once and shared with the GPU file."""

import types

import numpy as np
import pytest

from test_gpu_unionfind import random_syndromes
from test_unionfind import chain_graph, memory, syndrome_of

from tsim_amd import faults
from tsim_amd.decode import DecodingGraph, UnionFindDecoder, uf_shot_bytes

LDS_BLOCK, LDS_CU, MAX_WAVES = 64 * 1024, 160 * 1024, 4  # kLdsBlock, kLdsCU, kMaxWaves of csrc/tsim_uf.hip.h

CASES = ("d9", "d15", "dense", "fits", "fits_weighted", "three_waves", "chain1500")

# shots (waves) per block by the rule of tsim_uf_create (shots_per_block_rule below), worked out by hand per case:
# (case, weighted) -> waves.  E.g. chain1500: 12512 bytes a shot, 13 blocks of 1 wave on a CU against 3 blocks of 4 (12), so 1;
# with 4-bit counters 13072 bytes, 12 shots on a CU whichever way, and a tie goes to the most waves, so 4.
SHOTS_PER_BLOCK = {("d9", False): 1, ("d9", True): 1, ("d15", False): 1, ("d15", True): 1, ("dense", False): 2, ("dense", True): 1,
                   ("fits", False): 1, ("fits_weighted", True): 1, ("three_waves", False): 3, ("three_waves", True): 2,
                   ("chain1500", False): 1, ("chain1500", True): 4}

CHAIN_DEFECTS = ([400, 1100], [11, 1401], [701], [301, 601, 901], [750], [741, 761, 1201, 1221])  # nodes
CHAIN_ROWS = 75 * np.arange(len(CHAIN_DEFECTS))  # a tile of 64 rows each, on another lane each: the four waves of a block all decode


def shots_per_block_rule(shot_bytes: int) -> int:
    """The chooser of ``tsim_uf_create``: as many shots on a CU as its LDS holds (at most 32 waves), a tie to the most waves."""
    best = waves = 0
    for w in range(1, MAX_WAVES + 1):
        block = 16 + w * shot_bytes
        if block > LDS_BLOCK:
            break
        blocks = min(LDS_CU // block, 32 // w)
        if blocks * w >= best:
            best, waves = blocks * w, w
    return waves


def sorted_graph(n_nodes, u, v, obs) -> DecodingGraph:
    order = np.lexsort((v, u))
    return DecodingGraph(n_nodes, np.asarray(u)[order], np.asarray(v)[order], np.asarray(obs, np.uint64)[order])


def dense_graph(seed: int = 31, n_nodes: int = 400, n_edges: int = 65535) -> DecodingGraph:
    """A random subset of all pairs of ``n_nodes`` nodes (79800 at 400), boundary pairs ``(0, a)`` among them; masks 0 .. 3."""
    rng = np.random.default_rng(seed)
    u, v = np.triu_indices(n_nodes, 1)
    pick = np.sort(rng.choice(len(u), size=n_edges, replace=False))
    return sorted_graph(n_nodes, u[pick], v[pick], rng.integers(0, 4, size=n_edges))


def sparse_graph(seed: int, n_nodes: int, n_local: int, n_boundary: int, island: int = 0, extra_nodes: int = 0) -> DecodingGraph:
    """``n_local`` random edges ``(u, v)``, ``0 < v - u < 40``, among the nodes 1 .. ``n_nodes - island - 1``, ``n_boundary`` edges
    ``(0, a)`` to nodes of the same range, and the last ``island`` nodes joined in a path that nothing else touches (a component
    without a boundary edge); masks 0 .. 3.  ``extra_nodes`` more nodes without an edge follow."""
    rng = np.random.default_rng(seed)
    last = n_nodes - island  # the nodes 1 .. last - 1 carry the random edges
    u = np.repeat(np.arange(1, last), 39)
    v = u + np.tile(np.arange(1, 40), last - 1)
    ok = np.flatnonzero(v < last)
    pick = rng.choice(ok, size=n_local, replace=False)
    b = rng.choice(np.arange(1, last), size=n_boundary, replace=False)
    i = np.arange(last, n_nodes - 1)
    eu = np.concatenate([u[pick], np.zeros(n_boundary, np.int64), i])
    ev = np.concatenate([v[pick], b, i + 1])
    return sorted_graph(n_nodes + extra_nodes, eu, ev, rng.integers(0, 4, size=len(eu)))


def fits_graph(extra_nodes: int = 0) -> DecodingGraph:
    """7008 nodes, 30200 edges (944 bitmap words): 16 + 65520 bytes of LDS for the unweighted state, a block's 65536 exactly.
    7008 is a multiple of 16, so one more node lengthens every per-node array."""
    return sparse_graph(41, 7008, 29898, 300, island=3, extra_nodes=extra_nodes)


def fits_weighted_graph(extra_nodes: int = 0) -> DecodingGraph:
    """4624 nodes, 41472 edges (1296 bitmap words, 5184 counter words): 65520 bytes for the weighted state."""
    return sparse_graph(43, 4624, 41170, 300, island=3, extra_nodes=extra_nodes)


def random_caps(graph: DecodingGraph, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(1, 15, size=graph.n_edges).astype(np.uint8)


def defect_rows(rng, n: int, nd: int, n_obs: int, weight: int) -> np.ndarray:
    """``random_syndromes`` with at least one defect in every row."""
    bits = random_syndromes(rng, n, nd, n_obs, weight)
    for r in np.flatnonzero(~bits[:, :nd].any(axis=1)):
        bits[r, rng.integers(0, nd)] = True
    return bits


def island_rows(bits: np.ndarray, nd: int, island: int = 3) -> np.ndarray:
    """Rows 0 .. 2 meet the island (the last ``island`` detectors): one defect there (a miss), two (matched inside it), three."""
    bits[:, nd - island:nd] = False
    bits[0, nd - 2] = True
    bits[1, [nd - 3, nd - 1]] = True
    bits[2, nd - 3:nd] = True
    return bits


def surface_case(d: int, p: float, n: int):
    c = memory(d, p)
    form = c.compile_faults()
    bits = faults.fault_rows_host(form, 0, n, (1, 2)).view(np.bool_)
    plain = UnionFindDecoder.from_circuit(c)
    # what from_circuit(c, weights="probability") builds, without building the graph a second time
    return plain, UnionFindDecoder(plain.graph, plain.num_observables, plain.graph.growth_caps()), bits


_CASES: dict = {}


def case(name: str):
    """``plain`` / ``weighted`` (a decoder, or ``None`` where the case has none) and ``bits`` (bool rows: detectors, observables)."""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng(CASES.index(name) + 100)
    if name == "d9":
        plain, weighted, bits = surface_case(9, 0.01, 96)
    elif name == "d15":
        plain, weighted, bits = surface_case(15, 0.005, 48)
    elif name == "dense":
        g = dense_graph()
        plain, weighted = UnionFindDecoder(g, 2), UnionFindDecoder(g, 2, edge_caps=random_caps(g, 32))
        bits = defect_rows(rng, 128, g.n_nodes - 1, 2, 40)  # (two tiles: both waves of a block decode)
    elif name == "fits":
        g = fits_graph()
        plain, weighted = UnionFindDecoder(g, 2), None  # (the weighted state of this graph does not fit a block)
        bits = island_rows(random_syndromes(rng, 48, g.n_nodes - 1, 2, 300), g.n_nodes - 1)
    elif name == "fits_weighted":
        g = fits_weighted_graph()
        plain, weighted = None, UnionFindDecoder(g, 2, edge_caps=random_caps(g, 44))
        bits = island_rows(random_syndromes(rng, 48, g.n_nodes - 1, 2, 100), g.n_nodes - 1)
    elif name == "three_waves":
        g = sparse_graph(47, 2000, 6300, 100)
        plain, weighted = UnionFindDecoder(g, 2), UnionFindDecoder(g, 2, edge_caps=random_caps(g, 48))
        bits = random_syndromes(rng, 200, g.n_nodes - 1, 2, 60)
    else:
        g = chain_graph(1500, obs_edge=700)
        plain, weighted = UnionFindDecoder(g), UnionFindDecoder(g, edge_caps=np.resize([1, 14, 3, 8], 1499))
        bits = np.zeros((int(CHAIN_ROWS[-1]) + 1, 1500), np.bool_)  # (rows without a defect between them cost a wave nothing)
        for r, nodes in zip(CHAIN_ROWS, CHAIN_DEFECTS):
            bits[r, np.array(nodes) - 1] = True
        bits[:, 1499] = rng.integers(0, 2, size=len(bits)).astype(np.bool_)
    _CASES[name] = types.SimpleNamespace(name=name, plain=plain, weighted=weighted, bits=bits)
    return _CASES[name]


def decoders(c):
    """``(weighted?, decoder)`` for the decoders the case has."""
    return [(w, uf) for w, uf in ((False, c.plain), (True, c.weighted)) if uf is not None]


def shot_bytes(uf) -> int:
    return uf_shot_bytes(uf.graph.n_nodes, uf.graph.n_edges, uf.edge_caps is not None)


def most_words(uf, dets) -> int:
    """The most distinct 32-bit words of the edge bitmap that one row's correction touches (every flipped edge is full)."""
    return max(len(np.unique(e >> 5)) for e in uf.flipped_edges(dets))


# ---- the inputs reach the code ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_graphs_are_what_the_cases_say(name):
    c = case(name)
    for weighted, uf in decoders(c):
        g = uf.graph
        assert (g.edge_u < g.edge_v).all() and (np.diff(g.edge_u.astype(np.int64) * g.n_nodes + g.edge_v) > 0).all()
        assert c.bits.shape[1] == uf.num_detectors + uf.num_observables
        assert 16 + shot_bytes(uf) <= LDS_BLOCK
        assert SHOTS_PER_BLOCK[name, weighted] == shots_per_block_rule(shot_bytes(uf)), (name, weighted, shot_bytes(uf))
    sizes = {name: (uf.graph.n_nodes, uf.graph.n_edges) for _, uf in decoders(c)}[name]
    want = dict(d9=(721, 3534), d15=(3361, 17862), dense=(400, 65535), fits=(7008, 30200), fits_weighted=(4624, 41472),
                three_waves=(2000, 6400), chain1500=(1500, 1499))
    assert sizes == want[name]


def test_the_cases_cover_every_number_of_waves():
    """Wave ``w`` of block 0 owns tile ``w`` (rows ``64 w .. 64 w + 63``) and touches its state at ``16 + w * shot_bytes`` only for
    a row with a defect: every case has such a row in each of the first ``shots_per_block`` tiles."""
    assert set(SHOTS_PER_BLOCK.values()) == {1, 2, 3, 4}
    assert set(SHOTS_PER_BLOCK) == {(name, w) for name in CASES for w, _ in decoders(case(name))}
    assert 16380 < shot_bytes(case("three_waves").plain) <= 18199
    for (name, _), waves in SHOTS_PER_BLOCK.items():
        c = case(name)
        nd = decoders(c)[0][1].num_detectors
        assert -(-len(c.bits) // 64) >= waves
        assert all(c.bits[64 * w:64 * w + 64, :nd].any() for w in range(waves)), name


@pytest.mark.parametrize("name", CASES)
def test_every_correction_reproduces_its_syndrome(name):
    c = case(name)
    for _, uf in decoders(c):
        dets = c.bits[:, :uf.num_detectors]
        missed, flipped, pred = uf.missed(dets), uf.flipped_edges(dets), uf.predictions(dets)
        for r in np.flatnonzero(~missed):
            assert np.array_equal(syndrome_of(uf.graph, flipped[r]), dets[r]), (name, r)
            assert int(np.bitwise_xor.reduce(uf.graph.edge_obs[flipped[r]], initial=np.uint64(0))) == int(pred[r]), (name, r)
        assert not pred[missed].any() and all(len(flipped[r]) == 0 for r in np.flatnonzero(missed))


@pytest.mark.parametrize("name", ["d15", "fits", "fits_weighted"])
def test_more_than_64_listed_words(name):
    """A row whose flipped edges lie in more than 64 words of the bitmap has listed more than 64 words: lanes of
    ``full_edges()`` take a second word."""
    c = case(name)
    for weighted, uf in decoders(c):
        words = most_words(uf, c.bits[:, :uf.num_detectors])
        print(f"{name} weighted={weighted}: {words} words at most")
        assert words > 64


def test_dense_flips_edges_beyond_int16():
    c = case("dense")
    for weighted, uf in decoders(c):
        top = max(int(e.max()) for e in uf.flipped_edges(c.bits[:, :399]) if len(e))
        print(f"dense weighted={weighted}: largest flipped edge {top}")
        assert top >= 32768
    assert int(c.plain.graph.edge_u.min()) == 0  # boundary pairs are among the edges


def test_chain_has_hundreds_of_levels_and_thousands_of_rounds():
    """On a chain the flipped edges of a cluster are a path: 256 of them in one row are levels beyond 255."""
    c = case("chain1500")
    for weighted, uf in decoders(c):
        dets = c.bits[:, :1499]
        most = max(len(e) for e in uf.flipped_edges(dets))
        rounds = int(uf.growth_rounds(dets).max())
        print(f"chain1500 weighted={weighted}: {most} flipped edges, {rounds} growth rounds at most")
        assert most >= 256 and rounds >= 1024 and not uf.missed(dets).any()
    assert c.plain.flipped_edges(c.bits[:1, :1499])[0].tolist() == list(range(400, 1100))
    assert (CHAIN_ROWS // 64).tolist() == list(range(6)) and len(set((CHAIN_ROWS % 64).tolist())) == 6


@pytest.mark.parametrize("name", ["fits", "fits_weighted"])
def test_fits_has_a_miss_and_fills_the_block(name):
    c = case(name)
    (weighted, uf), = decoders(c)
    missed = uf.missed(c.bits[:, :uf.num_detectors])
    assert missed[0] and not missed[1] and missed[2] and not missed.all()
    spare = LDS_BLOCK - 16 - shot_bytes(uf)
    assert 0 <= spare < 16
    bigger = (fits_weighted_graph if weighted else fits_graph)(extra_nodes=1)
    assert (bigger.n_nodes, bigger.n_edges) == (uf.graph.n_nodes + 1, uf.graph.n_edges)
    assert np.array_equal(bigger.edge_u, uf.graph.edge_u) and np.array_equal(bigger.edge_v, uf.graph.edge_v)
    assert 16 + uf_shot_bytes(bigger.n_nodes, bigger.n_edges, weighted) > LDS_BLOCK
    if not weighted:
        assert 16 + uf_shot_bytes(uf.graph.n_nodes, uf.graph.n_edges, True) > LDS_BLOCK  # why `fits` has no weighted variant
