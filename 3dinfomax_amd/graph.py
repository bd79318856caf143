"""Batched molecular graph container.

Replaces the slice of DGL the hot path uses (`dgl.graph`, `dgl.batch`, `ndata`/`edata`,
`batch_num_nodes`, `number_of_nodes`, `edges`, `.to`) - see reference
datasets/custom_collate.py:105-114 (contrastive_collate -> dgl.batch) and
trainer/self_supervised_trainer.py:24-29 (what the trainer touches).

On top of the DGL-like surface it carries the index the HIP kernels are driven by
(`GraphIndex`): a CSR **by destination**.  All edge-sized tensors inside the models live
in *destination-sorted* order ("epos" order, stable w.r.t. edge id, so the per-node
message order equals DGL's mailbox order), which makes every neighbourhood a contiguous
row range `[in_ptr[v], in_ptr[v+1])` - the layout the one-pass segmented aggregation
kernel wants - and needs no atomics anywhere (out-edge sums go through `out_ptr/out_epos`).
"""
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch


@dataclass
class GraphIndex:
    """int32 index arrays, all on one device.  E edges, N nodes, B graphs."""
    num_nodes: int
    num_edges: int
    num_graphs: int
    in_ptr: torch.Tensor      # [N+1] CSR row pointer by destination
    perm: torch.Tensor        # [E]   epos -> edge id (stable sort of dst)
    src_s: torch.Tensor       # [E]   source node of edge at epos
    dst_s: torch.Tensor       # [E]   destination node of edge at epos (non-decreasing)
    out_ptr: torch.Tensor     # [N+1] CSR row pointer by source
    out_epos: torch.Tensor    # [E]   epos of the out-edges of each node, grouped by source
    graph_ptr: torch.Tensor   # [B+1] node offsets of the graphs in the batch
    inv_perm: torch.Tensor    # [E]   edge id -> epos
    max_in_degree: int
    # nodes grouped by in-degree (degree-combined posttrans weights, csrc/grouped.hip); built lazily by degree_groups()
    deg_rows: Optional[torch.Tensor] = None        # [M_pad] node ids grouped by in-degree, each group padded to 64 with -1
    deg_tile_group: Optional[torch.Tensor] = None  # [M_pad/64] group of every 64-row tile
    deg_groups: Optional[tuple] = None             # host: ((D, start, count), ...) for the in-degrees present (0 included)

    def to(self, device):
        out = GraphIndex(self.num_nodes, self.num_edges, self.num_graphs,
                         *[t.to(device, non_blocking=True) for t in
                           (self.in_ptr, self.perm, self.src_s, self.dst_s, self.out_ptr,
                            self.out_epos, self.graph_ptr, self.inv_perm)], self.max_in_degree)
        if self.deg_rows is not None:
            out.deg_rows = self.deg_rows.to(device, non_blocking=True)
            out.deg_tile_group = self.deg_tile_group.to(device, non_blocking=True)
            out.deg_groups = self.deg_groups
        return out

    def degree_groups(self):
        """(deg_rows, deg_tile_group, deg_groups), computed once per batch from in_ptr (host round trip only if the
        batch was not assembled through build_index / dataset.assemble, which fill them in on the host)."""
        if self.deg_rows is None:
            indeg = np.diff(self.in_ptr.cpu().numpy().astype(np.int64))
            rows, tiles, groups = group_nodes_by_degree(indeg, include_zero=True)
            dev = self.in_ptr.device
            self.deg_rows = torch.from_numpy(rows).to(dev)
            self.deg_tile_group = torch.from_numpy(tiles).to(dev)
            self.deg_groups = groups
        return self.deg_rows, self.deg_tile_group, self.deg_groups


def group_nodes_by_degree(indeg, pad=64, include_zero=False):
    """Node ids grouped by in-degree (ascending D, ascending node id), every group padded with -1 to a multiple of
    `pad` rows; tile -> group map; ((D, start, count), ...).  `include_zero`: nodes without in-edges form a group of their
    own (D = 0, scaler coefficients 0: their aggregate is a zero row) so that the groups cover EVERY node - what the batch
    index carries, because the fused posttrans GEMM takes its BatchNorm statistics from the grouped launch's epilogue."""
    indeg = np.asarray(indeg, dtype=np.int64)
    order = np.argsort(indeg, kind='stable')
    if not include_zero:
        order = order[indeg[order] > 0]
    degs, counts = np.unique(indeg[order], return_counts=True)
    padded = (counts + pad - 1) // pad * pad
    starts = np.cumsum(padded) - padded
    rows = np.full(int(padded.sum()), -1, dtype=np.int32)
    src_off = np.cumsum(counts) - counts
    dst_idx = np.repeat(starts - src_off, counts) + np.arange(order.shape[0])
    rows[dst_idx] = order.astype(np.int32)
    tiles = np.repeat(np.arange(degs.shape[0], dtype=np.int32), padded // pad)
    groups = tuple((int(d), int(s), int(c)) for d, s, c in zip(degs, starts, counts))
    return rows, tiles, groups


def build_index(src, dst, num_nodes, batch_num_nodes) -> GraphIndex:
    """Host-side (numpy) construction of the kernel index from an edge list."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    bnn = np.asarray(batch_num_nodes, dtype=np.int64)
    E = src.shape[0]
    perm = np.argsort(dst, kind='stable')
    src_s, dst_s = src[perm], dst[perm]
    indeg = np.bincount(dst, minlength=num_nodes)
    in_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(indeg, out=in_ptr[1:])
    out_epos = np.argsort(src_s, kind='stable')
    out_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=num_nodes), out=out_ptr[1:])
    graph_ptr = np.zeros(bnn.shape[0] + 1, dtype=np.int64)
    np.cumsum(bnn, out=graph_ptr[1:])
    inv_perm = np.empty(E, dtype=np.int64)
    inv_perm[perm] = np.arange(E)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)))
    rows, tiles, groups = group_nodes_by_degree(indeg, include_zero=True)
    return GraphIndex(int(num_nodes), int(E), int(bnn.shape[0]), i32(in_ptr), i32(perm), i32(src_s),
                      i32(dst_s), i32(out_ptr), i32(out_epos), i32(graph_ptr), i32(inv_perm),
                      int(indeg.max()) if E else 0, torch.from_numpy(rows), torch.from_numpy(tiles), groups)


class BatchedMolGraph:
    """A (batch of) graph(s) with DGL's node/edge-frame surface."""

    def __init__(self, src, dst, num_nodes: int, batch_num_nodes=None,
                 ndata: Optional[Dict[str, torch.Tensor]] = None,
                 edata: Optional[Dict[str, torch.Tensor]] = None,
                 index: Optional[GraphIndex] = None):
        self._src = torch.as_tensor(src, dtype=torch.long)
        self._dst = torch.as_tensor(dst, dtype=torch.long)
        self._n = int(num_nodes)
        if batch_num_nodes is None:
            batch_num_nodes = torch.tensor([self._n], dtype=torch.long)
        self._bnn = torch.as_tensor(batch_num_nodes, dtype=torch.long)
        self.ready_event = None
        self.ndata: Dict[str, torch.Tensor] = dict(ndata or {})
        self.edata: Dict[str, torch.Tensor] = dict(edata or {})
        self._index = index

    # ---- DGL-like surface --------------------------------------------------------------
    def number_of_nodes(self):
        return self._n

    num_nodes = number_of_nodes

    def number_of_edges(self):
        return int(self._src.shape[0])

    num_edges = number_of_edges

    def edges(self):
        return self._src, self._dst

    def batch_num_nodes(self):
        return self._bnn

    @property
    def batch_size(self):
        return int(self._bnn.shape[0])

    @property
    def device(self):
        return self._src.device

    def to(self, device):
        device = torch.device(device)
        g = BatchedMolGraph(self._src.to(device), self._dst.to(device), self._n, self._bnn.to(device),
                            {k: v.to(device) for k, v in self.ndata.items()},
                            {k: v.to(device) for k, v in self.edata.items()},
                            self.index().to(device))
        if device.type == 'cuda':
            g.mark_ready()
        return g

    def mark_ready(self):
        """Record that everything this batch consists of has been enqueued on the current stream (streams.py: lets an
        independent consumer on another stream wait for the batch only)."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self._src.device))
        self.ready_event = ev

    def local_copy(self):
        """Same structure and tensors, fresh frames: the forward pass overwrites ndata/edata['feat'] (reference
        models/pna.py:162-163), so a resident batch that is stepped on repeatedly is forwarded through a copy."""
        g = BatchedMolGraph(self._src, self._dst, self._n, self._bnn, dict(self.ndata), dict(self.edata),
                            self._index)
        g.ready_event = self.ready_event
        return g

    def remove_nodes(self, nids) -> 'BatchedMolGraph':
        """DGL's `remove_nodes` semantics, returned as a NEW graph (DGL changes the graph in place; this one leaves `self` and
        its frames untouched): the kept nodes are renumbered in ascending order, every edge that touches a removed node is
        dropped, the kept edges keep their relative order, ndata / edata are sliced to match, and on a batched graph
        batch_num_nodes loses every molecule's removed nodes.  The kernel index is rebuilt on first use."""
        nids = torch.as_tensor(nids, dtype=torch.long).reshape(-1).to(self._src.device)
        keep = torch.ones(self._n, dtype=torch.bool, device=self._src.device)
        keep[nids] = False
        new_id = torch.cumsum(keep.long(), 0) - 1
        ek = keep[self._src] & keep[self._dst]
        bnn = self._bnn
        if nids.numel():
            mol = torch.repeat_interleave(torch.arange(bnn.shape[0], device=bnn.device), bnn)
            gone = ~keep.to(bnn.device)
            bnn = bnn - torch.bincount(mol[gone], minlength=bnn.shape[0])
        return BatchedMolGraph(new_id[self._src[ek]], new_id[self._dst[ek]], int(keep.sum()), bnn,
                               {k: v[keep] for k, v in self.ndata.items()}, {k: v[ek] for k, v in self.edata.items()})

    # ---- kernel index -----------------------------------------------------------------
    def index(self) -> GraphIndex:
        if self._index is None:
            idx = build_index(self._src.cpu().numpy(), self._dst.cpu().numpy(), self._n,
                              self._bnn.cpu().numpy())
            self._index = idx.to(self._src.device)
        return self._index


def batch(graphs: List[BatchedMolGraph]) -> BatchedMolGraph:
    """Block-diagonal batching (DGL `dgl.batch` semantics): nodes and
    edges concatenated in list order, node ids offset, frames concatenated,
    batch_num_nodes flattened."""
    srcs, dsts, bnn = [], [], []
    off = 0
    # items may be DGL-like graphs (the reference's own datasets yield `dgl.DGLGraph`s and `from infomax3d_amd import *`
    # rebinds the collate functions that land here): duck-typed through as_batched_graph, frames shared
    graphs = [as_batched_graph(g) for g in graphs]
    for g in graphs:
        srcs.append(g._src + off)
        dsts.append(g._dst + off)
        bnn.append(g._bnn)
        off += g._n
    out = BatchedMolGraph(torch.cat(srcs), torch.cat(dsts), off, torch.cat(bnn))
    for k in graphs[0].ndata:
        out.ndata[k] = torch.cat([g.ndata[k] for g in graphs], 0)
    for k in graphs[0].edata:
        out.edata[k] = torch.cat([g.edata[k] for g in graphs], 0)
    return out


def bond_graph(mol) -> BatchedMolGraph:
    """2D bond graph of one `synth.Molecule` (reference datasets/qm9_dataset.py:221-231)."""
    return BatchedMolGraph(torch.from_numpy(mol.src), torch.from_numpy(mol.dst), mol.n_atoms,
                           ndata={'feat': torch.from_numpy(mol.atom_feat)},
                           edata={'feat': torch.from_numpy(mol.bond_feat)})


def complete_graph(mol, coords=None, coordinates=False) -> BatchedMolGraph:
    """Complete 3D distance graph of one molecule (reference datasets/qm9_dataset.py:233-244).  coordinates=True: the atom
    positions as well, ndata['x'] float32 [n, 3] (:240) - what EGNN and the distance column of PNA read."""
    from .synth import complete_graph_edges, pairwise_distances
    coords = mol.coords if coords is None else coords
    src, dst = complete_graph_edges(mol.n_atoms)
    d = pairwise_distances(coords, src, dst)
    ndata = {'feat': torch.from_numpy(mol.atom_feat)}
    if coordinates:
        ndata['x'] = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.float32)).reshape(-1, 3)
    return BatchedMolGraph(torch.from_numpy(src), torch.from_numpy(dst), mol.n_atoms, ndata=ndata,
                           edata={'d': torch.from_numpy(d)})


def san_laplacian(mol, self_loops=True):
    """The [n, n] float32 matrix whose eigen-decomposition is SAN's positional encoding, as torch.linalg.eigh reads it (the lower
    triangle, mirrored).  The reference's lines as written (datasets/ogbg_dataset_extension.py:115-124 with self_loops, A + I;
    datasets/qm9_dataset.py:405-409 without): D = diag(colsum A), L = D - A, N = D ** -0.5 and `eye - N * L * N` with N a VECTOR,
    so both factors scale the columns: entry (i, j) is delta_ij - L_ij / D_j, and eigh takes i >= j of it.  An atom without bonds
    (self_loops=False) gets D = 1 as in the ogbg lines (the qm9 lines would give NaN)."""
    n = mol.n_atoms
    A = torch.zeros(n, n)
    if mol.src.shape[0]:
        A[torch.from_numpy(mol.src), torch.from_numpy(mol.dst)] = 1.0
    if self_loops:
        A = A + torch.eye(n)
    D = A.sum(dim=0)
    L = torch.diag(D) - A
    D = D + (D == 0)
    N = D ** -0.5
    M = torch.eye(n) - N * L * N
    low = torch.tril(M)
    return low + torch.tril(M, -1).T


def laplacian_pos_enc(mol, num_freq=10, self_loops=True, normalize=True):
    """SAN's Laplacian positional encoding of one `synth.Molecule`, host only -> float32 [n, num_freq, 2]: (eigenvalue,
    eigenvector entry) of the num_freq lowest eigenvalues of san_laplacian(mol, self_loops) (torch.linalg.eigh), eigenvalues
    ascending, the eigenvector matrix row-normalised (F.normalize over the kept eigenvectors; normalize=False: as eigh returns
    them), NaN-padded when n < num_freq, no sign flip.  Reference datasets/ogbg_dataset_extension.py:108-137 (self_loops=True)
    and datasets/qm9_dataset.py:403-419 (self_loops=False)."""
    n = mol.n_atoms
    eig_vals, eig_vecs = torch.linalg.eigh(san_laplacian(mol, self_loops))
    keep = eig_vals.argsort()[:num_freq]
    eig_vals, eig_vecs = eig_vals[keep], eig_vecs[:, keep]
    eig_vecs = eig_vecs[:, eig_vals.argsort()]
    if normalize:
        eig_vecs = torch.nn.functional.normalize(eig_vecs, p=2, dim=1, eps=1e-12)
    if n < num_freq:
        eig_vecs = torch.nn.functional.pad(eig_vecs, (0, num_freq - n), value=float('nan'))
        eig_vals = torch.nn.functional.pad(eig_vals, (0, num_freq - n), value=float('nan'))
    return torch.stack([eig_vals.unsqueeze(0).repeat(n, 1), eig_vecs], dim=-1)


def san_graph(mol, num_freq=10, sign_flip=None, self_loops=True) -> BatchedMolGraph:
    """SAN's input graph of one molecule (reference datasets/ogbg_dataset_extension.py:60-96): the complete graph without self
    loops in the reference's edge order (synth.complete_graph_edges); edata['feat'] int64 [E, 3] = the bond features on the real
    edges, zeros elsewhere; edata['real'] int64 [E] = 1 on the real edges; ndata['feat'] the atom features; ndata['pos_enc']
    [n, num_freq, 2] = laplacian_pos_enc.  sign_flip: one draw `torch.rand(num_freq) >= 0.5` -> +1 / -1 per eigenvector under the
    caller's seed, multiplied into the eigenvector entries (the reference draws these signs, :66-68, and then drops them); None /
    False: no draw."""
    from .synth import complete_graph_edges
    n = mol.n_atoms
    src, dst = complete_graph_edges(n)
    E = src.shape[0]
    feat = torch.zeros(E, mol.bond_feat.shape[1], dtype=torch.long)
    real = torch.zeros(E, dtype=torch.long)
    if mol.src.shape[0]:
        s, d = torch.from_numpy(mol.src), torch.from_numpy(mol.dst)
        pos = s * (n - 1) + d - (d > s).long()
        feat[pos] = torch.from_numpy(mol.bond_feat)
        real[pos] = 1
    pe = laplacian_pos_enc(mol, num_freq, self_loops)
    if sign_flip:
        flip = torch.rand(num_freq)
        flip = torch.where(flip >= 0.5, 1.0, -1.0)
        pe = torch.stack([pe[:, :, 0], pe[:, :, 1] * flip], dim=-1)
    return BatchedMolGraph(torch.from_numpy(src), torch.from_numpy(dst), n,
                           ndata={'feat': torch.from_numpy(mol.atom_feat), 'pos_enc': pe},
                           edata={'feat': feat, 'real': real})


def contrastive_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:105-114 (items may be BatchedMolGraphs or DGL-like graphs)."""
    graphs, graphs3d, *targets = map(list, zip(*batch_items))
    if targets:
        return [batch(graphs)], [batch(graphs3d)], torch.stack(*targets).float()
    return [batch(graphs)], [batch(graphs3d)]


def conformer_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:155-157."""
    graphs, confs = map(list, zip(*batch_items))
    return [batch(graphs)], [batch(confs)]


def graph_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:12-18 (the collate of the fine-tuning configs, e.g.
    configs_clean/tune_QM9_homo.yml): ([batched graph], targets [B, T]); 1-d targets get a trailing axis."""
    graphs, targets = map(list, zip(*batch_items))
    targets = torch.stack(targets).float()
    if len(targets.shape) == 1:
        targets = targets.unsqueeze(-1)
    return [batch(graphs)], targets


def pairwise_distance_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:65-78: items (graph, pairwise_indices [2, p], distances [p, 1]) ->
    ([batched graph, pairwise_indices [2, P] with every molecule's node offset added, mask [B, maxN] True on padding],
    distances [P, 1]).  The items' index tensors are not modified."""
    graphs, pairwise_indices, distances = map(list, zip(*batch_items))
    g = batch(graphs)
    n_atoms = g.batch_num_nodes()
    offsets = torch.cumsum(n_atoms, 0) - n_atoms
    pidx = torch.cat([torch.as_tensor(p) + off for p, off in zip(pairwise_indices, offsets.tolist())], dim=-1)
    mask = torch.arange(int(n_atoms.max()), device=distances[0].device)[None, :] >= n_atoms[:, None]
    return [g, pidx, mask], torch.cat(distances)


def contrastive_vae_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:52-63 (the 3D autoencoder's collate): items (graph, graph3d,
    pairwise_indices [2, p], distances [p, 1]) -> ([batched graph], [batched 3D graph, pairwise_indices [2, P] with every
    molecule's node offset added], distances [P, 1]).  Unlike the reference, which adds the offsets in place, the items' index
    tensors are not modified."""
    graphs, graphs3d, pairwise_indices, distances = map(list, zip(*batch_items))
    g = batch(graphs)
    n_atoms = g.batch_num_nodes()
    offsets = torch.cumsum(n_atoms, 0) - n_atoms
    pidx = torch.cat([torch.as_tensor(p) + off for p, off in zip(pairwise_indices, offsets.tolist())], dim=-1)
    return [g], [batch(graphs3d), pidx], torch.cat(distances)


class NodeDropCollate:
    """Mirror of reference datasets/custom_collate.py:230-263 (the GraphCL baseline's collate): items are tuples whose first
    field is the graph (BatchedMolGraph or DGL-like); for every graph of view 1 in item order, then for every graph of view 2,
    `torch.randperm(n)` is drawn and its first int(drop_ratio * n) nodes are removed -> ([batched view 1], [batched view 2]).
    Under the same torch seed the views are exactly the reference's.  Unlike the reference, which removes view 1's nodes
    from the caller's graphs in place, the items are left unmodified.  The fast path that builds the views on the device
    from one upload is dataset.BatchStream(..., node_drop=r)."""

    def __init__(self, drop_ratio):
        self.drop_ratio = drop_ratio

    def __call__(self, batch_items):
        graphs = [as_batched_graph(item[0]) for item in batch_items]
        device = graphs[0].device
        removed = []
        for _view in range(2):
            for g in graphs:
                n_atoms = g.number_of_nodes()
                perm = torch.randperm(n_atoms, device=device)
                removed.append(perm[:int(self.drop_ratio * n_atoms)])
        B = len(graphs)
        view1 = [g.remove_nodes(r) for g, r in zip(graphs, removed[:B])]
        view2 = [g.remove_nodes(r) for g, r in zip(graphs, removed[B:])]
        return [batch(view1)], [batch(view2)]


def _distance_key(g3, who):
    """The edge column the noising collates work on: 'w' where the 3D graph has it (what the reference's collates name),
    otherwise 'd' (what the reference's datasets and Net3D, and this package's complete_graph, Net3D and EGNN name)."""
    for key in ('w', 'd'):
        if key in g3.edata:
            return key
    raise KeyError(f"{who}: the 3D graphs carry neither edata['w'] nor edata['d'] (complete_graph(mol) sets 'd')")


class _NoisedCollate:
    def __init__(self, std, num_noised):
        self.std = std
        self.num_noised = num_noised

    def _check(self, g3):
        pass

    def _noised_copy(self, g3, key):
        raise NotImplementedError

    def __call__(self, batch_items):
        graphs, graphs3d, *targets = map(list, zip(*batch_items))
        g3 = batch(graphs3d)
        key = _distance_key(g3, type(self).__name__)
        self._check(g3)
        noised = [g3] + [self._noised_copy(g3, key) for _ in range(self.num_noised)]
        out = [batch(graphs)], [batch(noised)]
        if targets:
            return (*out, torch.stack(*targets).float())
        return out


class NoisedDistancesCollate(_NoisedCollate):
    """Mirror of reference datasets/custom_collate.py:131-152 (the collate of configs/old_configs/contrastive_training_noised_3d.yml,
    the producer of NTXentExtraNegatives' z2): items (graph, graph3d[, target]) -> ([batched 2D], [batched 3D of (1 + num_noised) B
    molecules])[, stacked targets].  The 3D batch is the clean batch followed by num_noised copies of it whose distance column is
    `w + torch.randn_like(w) * std`, one draw of the whole batched column per copy, in copy order: under the same torch seed the
    copies are exactly the reference's.  Copy-major: molecule i of copy c is graph c B + i (the order the loss's [B, U, D] view of
    z2[B:] is paired with in the reference, kept as it is).  No clamp: a noised distance may be negative.
    The edge key: the reference noises edata['w'], which its own datasets and Net3D do not use (they name the distance 'd'); here
    'w' is noised when the 3D graphs have it - reference-exact - and otherwise 'd', the column complete_graph, Net3D and EGNN use.
    Items may be BatchedMolGraphs or DGL-like graphs and are left unmodified.  The fast path that builds the copies on the device
    from the clean batch's upload is dataset.BatchStream(..., noised_3d={...})."""

    def _noised_copy(self, g3, key):
        w = g3.edata[key]
        edata = dict(g3.edata)
        edata[key] = w + torch.randn_like(w) * self.std
        return BatchedMolGraph(g3._src, g3._dst, g3._n, g3._bnn, dict(g3.ndata), edata)


class NoisedCoordinatesCollate(_NoisedCollate):
    """Mirror of reference datasets/custom_collate.py:160-185: as NoisedDistancesCollate, but every copy's positions are
    `x + torch.randn_like(x) * std` (one draw of the batched ndata['x'] per copy, in copy order: the reference's draws under
    the same torch seed), the copy keeps the noised ndata['x'], and the distance of every edge is recomputed from them
    (torch.norm(x[src] - x[dst], p=2, dim=-1)[:, None]) into the distance column ('w' when the graphs have it, otherwise 'd': see
    NoisedDistancesCollate).  The 3D graphs must carry ndata['x'] (complete_graph(mol, coordinates=True))."""

    def _check(self, g3):
        if 'x' not in g3.ndata:
            raise ValueError("NoisedCoordinatesCollate needs the atom coordinates in ndata['x'] of the 3D graphs "
                             "(complete_graph(mol, coordinates=True))")

    def _noised_copy(self, g3, key):
        x = g3.ndata['x']
        x = x + torch.randn_like(x) * self.std
        ndata, edata = dict(g3.ndata), dict(g3.edata)
        ndata['x'] = x
        edata[key] = torch.norm(x[g3._src] - x[g3._dst], p=2, dim=-1)[:, None]
        return BatchedMolGraph(g3._src, g3._dst, g3._n, g3._bnn, ndata, edata)


def _snorm_n(graphs):
    """sqrt(1 / n_atoms) per node, [N, 1] (reference datasets/custom_collate.py:45-47, 96-98: the graph-size
    normalisation factor of the original PNA, models/pna_original.py:258-259)."""
    sizes = [as_batched_graph(g).number_of_nodes() for g in graphs]
    return torch.cat([torch.full((n, 1), 1.0 / float(n), dtype=torch.float32) for n in sizes]).sqrt()


def s_norm_graph_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:43-49: ([batched graph, snorm_n], targets)."""
    graphs, targets = map(list, zip(*batch_items))
    return [batch(graphs), _snorm_n(graphs)], torch.stack(targets).float()


def s_norm_contrastive_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:93-102: ([batched graph, snorm_n], [batched 3D graph])."""
    graphs, graphs3d = map(list, zip(*batch_items))
    return [batch(graphs), _snorm_n(graphs)], [batch(graphs3d)]


class GeometricBatch:
    """What SMP reads of a torch_geometric Batch of Data(z=..., pos=...) objects: z [N, F] int64, pos [N, 3] fp32, batch [N] int64
    (the molecule of every atom, non-decreasing) and num_graphs, with .to(device).  Built without PyG."""

    def __init__(self, z, pos, batch, num_graphs):
        self.z, self.pos, self.batch, self.num_graphs = z, pos, batch, int(num_graphs)

    @classmethod
    def from_data_list(cls, items):
        """items: objects with .z and .pos (PyG Data), or synth.Molecule (atom_feat, coords)"""
        zs = [torch.as_tensor(it.z if hasattr(it, 'z') else it.atom_feat) for it in items]
        ps = [torch.as_tensor(it.pos if hasattr(it, 'pos') else it.coords, dtype=torch.float32) for it in items]
        sizes = torch.tensor([p.shape[0] for p in ps], dtype=torch.long)
        return cls(torch.cat(zs), torch.cat(ps), torch.repeat_interleave(torch.arange(len(items)), sizes), len(items))

    def to(self, device, non_blocking=False):
        return GeometricBatch(self.z.to(device, non_blocking=non_blocking), self.pos.to(device, non_blocking=non_blocking),
                              self.batch.to(device, non_blocking=non_blocking), self.num_graphs)

    @property
    def num_nodes(self):
        return self.pos.shape[0]


def pytorch_geometric_collate(batch_items):
    """Mirror of reference datasets/custom_collate.py:24-27 (the collate of sphere_net.yml and the SMP_*_conformers configs): items
    (data, target) -> ([GeometricBatch], targets [B, T]).  Items (graph, data) without a tensor in second place give the pair form of
    pytorch_geometric3d_contrastive_collate (:117-121, the contrastive SMP config): ([batched graph], [GeometricBatch])."""
    first, second = map(list, zip(*batch_items))
    if torch.is_tensor(second[0]):
        return [GeometricBatch.from_data_list(first)], torch.stack(second).float()
    return [batch(first)], [GeometricBatch.from_data_list(second)]


def as_batched_graph(g) -> BatchedMolGraph:
    """Accept a BatchedMolGraph, or any DGL-like object exposing edges(), number_of_nodes(),
    batch_num_nodes(), ndata, edata (real `dgl.DGLGraph` included).  The frames are shared,
    so the forward pass's side effects (reference models/pna.py:162-163,213) land on the
    caller's object."""
    if isinstance(g, BatchedMolGraph):
        return g
    cached = getattr(g, '_amd_batched', None)
    if cached is not None:
        return cached
    src, dst = g.edges()
    bg = BatchedMolGraph(src, dst, g.number_of_nodes(), g.batch_num_nodes())
    bg.ndata = g.ndata
    bg.edata = g.edata
    try:
        g._amd_batched = bg
    except Exception:
        pass
    return bg
