"""Python twin of the reference's ``gpusim::FingerprintDB`` (fingerprintdb_cuda.h:53-140)
over the C ABI: same method names, argument meaning and error behaviour, so the
parity tests read like test/test_gpusim.cpp.  The C++ twin used by the server is
gpusimilarity_amd/csrc/host/fingerprintdb.h.

Strings (SMILES / IDs) live here, above the ABI; the ABI speaks row indices.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import capi


def get_gpu_count() -> int:
    """fingerprintdb_cuda.cu:40-52"""
    return capi.device_count()


def get_next_gpu(required_memory: int) -> int:
    """fingerprintdb_cuda.cu:54-68 (throws when no GPU has room)"""
    return capi.next_device(required_memory)


def get_available_gpu_memory() -> int:
    """fingerprintdb_cuda.cu:401-413"""
    return capi.available_device_bytes()


class FingerprintDB:
    def __init__(self, fp_bitcount: int, fp_count: int, dbkey: str, data: Sequence[np.ndarray],
                 smiles_vector: List[bytes], ids_vector: List[bytes]):
        """fingerprintdb_cuda.cu:133-166.  ``data``: one uint32 [rows, W] array (or raw
        bytes) per storage block."""
        if fp_bitcount % 32 != 0:
            raise ValueError("fingerprint size must be a multiple of 32 bits")
        self.m_fp_intsize = fp_bitcount // 32
        self.m_total_count = fp_count
        self.m_dbkey = dbkey
        self.m_fold_factor = 1
        self._table = capi.Table(fp_bitcount)
        current = 0
        for block in data:
            if isinstance(block, (bytes, bytearray, memoryview)):
                block = np.frombuffer(block, dtype="<u4")
            block = np.ascontiguousarray(block, dtype=np.uint32).reshape(-1, self.m_fp_intsize)
            self._table.add_rows(block)
            current += block.shape[0]
        if current != fp_count:
            # fingerprintdb_cuda.cu:153-156
            raise RuntimeError("Mismatch between FP count and data, potential database corruption.")
        self.m_total_data_size = fp_count * self.m_fp_intsize * 4
        # the reference steals the callers' vectors (:164-165)
        self.m_smiles = list(smiles_vector)
        self.m_ids = list(ids_vector)
        smiles_vector.clear()
        ids_vector.clear()
        self._on_gpu = False

    def copyToGPU(self, fold_factor: int = 1, device: int = -1, ndevices: int = 1):
        """fingerprintdb_cuda.cu:168-195.  fold_factor > 1 keeps an OR-folded copy on the
        GPU and makes search() the reference's approximate folded search (re-scored with
        the full fingerprints); the effective factor is the smallest one >= fold_factor
        that divides the word count (:170-173)."""
        if fold_factor > 1:
            self._table.set_fold_factor(fold_factor)
        self._table.finalize(device, ndevices)
        self.m_fold_factor = self._table.fold_factor()
        self._on_gpu = True

    def count(self) -> int:
        return self.m_total_count

    def getFingerprint(self, index: int) -> np.ndarray:
        """fingerprintdb_cuda.cu:212-226"""
        return self._table.row(index)

    def getSmiles(self, index: int) -> bytes:
        return self.m_smiles[index]

    def getID(self, index: int) -> bytes:
        return self.m_ids[index]

    def getFingerprintDataSize(self) -> int:
        return self.m_total_data_size

    def getFingerprintBitcount(self) -> int:
        return self.m_fp_intsize * 32

    def search(self, query, dbkey: str, max_return_count: int, similarity_cutoff: float
               ) -> Tuple[List[bytes], List[bytes], List[float], int]:
        """fingerprintdb_cuda.cu:341-381 -> (smiles, ids, scores, approximate_result_count).
        Wrong dbkey: empty result (:349-352)."""
        if dbkey != self.m_dbkey:
            return [], [], [], 0
        hits, approx = self._table.search(np.asarray(query, dtype=np.uint32), max_return_count,
                                          float(similarity_cutoff))
        h = hits[0]
        return ([self.m_smiles[r] for r in h["row"]], [self.m_ids[r] for r in h["row"]],
                [float(s) for s in h["score"]], int(approx[0]))

    def search_hits(self, query, max_return_count: int, similarity_cutoff: float = 0.0, **kw):
        """Row-level result (row, score, common, popc_db) -- what the ABI returns."""
        hits, approx = self._table.search(np.asarray(query, dtype=np.uint32), max_return_count,
                                          float(similarity_cutoff), **kw)
        return hits[0], int(approx[0])

    def neighbors(self, cutoff: float, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0, beta: float = 1.0,
                  row_begin: int = 0, row_end=None):
        """Every pair of rows at or above `cutoff` (gsim_db_neighbors) -> CSR (indptr, indices, scores) for the rows
        [row_begin, row_end), each row's list sorted by column.  No counterpart in the reference."""
        return self._table.neighbors(float(cutoff), metric, alpha, beta, row_begin, row_end)

    def knn(self, k: int, cutoff: float, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0, beta: float = 1.0,
            row_begin: int = 0, row_end=None):
        """Each row's k most similar other rows at or above `cutoff` (gsim_db_knn) -> CSR (indptr, indices, scores) for the rows
        [row_begin, row_end), each row's list by (score descending, row ascending).  No counterpart in the reference."""
        return self._table.knn(int(k), float(cutoff), metric, alpha, beta, row_begin, row_end)

    def knn_join(self, left, k: int, cutoff: float, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0, beta: float = 1.0,
                 row_begin: int = 0, row_end=None, exclude_self: bool = False):
        """Each left row's k most similar rows of this table at or above `cutoff` (gsim_db_knn_join / gsim_db_knn_queries) -> CSR
        (indptr, indices, scores), each list by (score descending, row ascending).  `left`: another FingerprintDB on the same GPU
        (its rows [row_begin, row_end)), or an array of fingerprints.  `exclude_self` (only with left = this object): a row is not
        its own neighbour -- knn's lists.  No counterpart in the reference."""
        if isinstance(left, FingerprintDB):
            left = left._table
        return self._table.knn_join(left, int(k), float(cutoff), metric, alpha, beta, row_begin, row_end, exclude_self)

    def join(self, left, cutoff: float, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0, beta: float = 1.0,
             order: int = capi.JOIN_BY_ROW, row_begin: int = 0, row_end=None):
        """Every row of this table at or above `cutoff`, per left row (gsim_db_join / gsim_db_join_queries) -> CSR
        (indptr, indices, scores).  `left`: another FingerprintDB on the same GPU, or an array of fingerprints."""
        if isinstance(left, FingerprintDB):
            left = left._table
        return self._table.join(left, float(cutoff), metric, alpha, beta, order, row_begin, row_end)

    def screen(self, query):
        """The fingerprint screen of a substructure search: the rows whose bits include all of `query`'s (Tversky 1 / 0 = 1.0)."""
        return self.join(query, 1.0, capi.METRIC_TVERSKY, 1.0, 0.0)[1]

    def butina(self, cutoff: float, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0, beta: float = 1.0):
        """Taylor-Butina clustering at `cutoff` -> one tuple per cluster in creation order: the centroid first, then
        its members ascending (the shape of RDKit's Butina.ClusterData result)."""
        indptr, indices, _ = self.neighbors(cutoff, metric, alpha, beta)
        cluster_of, centroids = capi.butina(indptr, indices)
        members = [[] for _ in range(len(centroids))]
        for r, c in enumerate(cluster_of.tolist()):
            if r != centroids[c]:
                members[c].append(r)
        return [(int(c),) + tuple(m) for c, m in zip(centroids.tolist(), members)]

    def maxmin(self, npicks: int, seeds=(), metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0, beta: float = 1.0,
               max_score: float = 1.0, assign: bool = False):
        """MaxMin diversity picking (gsim_db_maxmin) -> the picked rows, in pick order.  assign=True: (picks, clusters),
        one tuple per pick -- the pick first, then the rows whose nearest pick it is, ascending (the shape of butina())."""
        out = self._table.maxmin(int(npicks), seeds, metric, alpha, beta, float(max_score), assign)
        picks = out[0].tolist()
        if not assign:
            return picks
        members = [[] for _ in picks]
        for r, j in enumerate(out[3].tolist()):
            if r != picks[j]:
                members[j].append(r)
        return picks, [(p,) + tuple(m) for p, m in zip(picks, members)]

    def leader(self, cutoff: float, seeds=(), max_leaders=None, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0,
               beta: float = 1.0, assign: bool = False):
        """Leader (sphere-exclusion) clustering (gsim_db_leader) -> the leaders, in the order they were made.  assign=True:
        (leaders, clusters), one tuple per leader -- the leader first, then the rows it covers, ascending (the shape of butina());
        rows a cap left unassigned are in no cluster."""
        leaders, leader_of, _, _ = self._table.leader(float(cutoff), seeds, max_leaders, assign, metric, alpha, beta)
        leaders = leaders.tolist()
        if not assign:
            return leaders
        members = [[] for _ in leaders]
        for r, j in enumerate(leader_of.tolist()):
            if j != capi.LEADER_NONE and r != leaders[j]:
                members[j].append(r)
        return leaders, [(p,) + tuple(m) for p, m in zip(leaders, members)]

    def dbscan(self, cutoff: float, min_pts: int, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0, beta: float = 1.0):
        """DBSCAN density clustering (gsim_db_dbscan) -> (clusters, noise): one tuple per cluster, in ascending order of its smallest
        core row -- that row first, then the other members (cores and border rows), ascending (the shape of butina()); `noise` is the
        list of the rows in no cluster.  A row is a core when it and its neighbours at `cutoff` are at least `min_pts` rows."""
        label_of, _, _, first_row, _, _ = self._table.dbscan(float(cutoff), int(min_pts), metric, alpha, beta, degree=False, anchor=False,
                                                             sizes=False)
        first = first_row.tolist()
        members = [[] for _ in first]
        noise = []
        for r, c in enumerate(label_of.tolist()):
            if c == capi.DBSCAN_NOISE:
                noise.append(r)
            elif r != first[c]:
                members[c].append(r)
        return [(f,) + tuple(m) for f, m in zip(first, members)], noise

    def jarvis_patrick(self, k: int, kmin: int, cutoff: float = 1e-45, metric: int = capi.METRIC_TANIMOTO, alpha: float = 1.0,
                       beta: float = 1.0, closed: bool = False, either: bool = False):
        """Jarvis-Patrick clustering (gsim_db_jarvis_patrick): two rows are joined when each is among the other's k nearest
        neighbours (either=True: one of them suffices) and their neighbour lists share at least `kmin` rows (closed=True: a list
        counts its owner) -> one tuple per cluster, in ascending order of its smallest row -- that row first, then the other
        members, ascending (the shape of butina()).  The default cutoff, the smallest positive float, lists every row with a
        non-zero score."""
        levels, _ = self._table.jarvis_patrick(int(k), [int(kmin)], float(cutoff), metric, alpha, beta, closed, either, sizes=False)
        cluster_of, first_row, _ = levels[0]
        first = first_row.tolist()
        members = [[] for _ in first]
        for r, c in enumerate(cluster_of.tolist()):
            if r != first[c]:
                members[c].append(r)
        return [(f,) + tuple(m) for f, m in zip(first, members)]

    def search_cpu(self, query, dbkey: str, max_return_count: int, similarity_cutoff: float
                   ) -> Tuple[List[bytes], List[bytes], List[float]]:
        """fingerprintdb_cuda.cpp:20-54 (cutoff ignored, approx not produced)."""
        if dbkey != self.m_dbkey:
            return [], [], []
        h = self._table.search_cpu(np.asarray(query, dtype=np.uint32), max_return_count, float(similarity_cutoff))[0]
        return ([self.m_smiles[r] for r in h["row"]], [self.m_ids[r] for r in h["row"]],
                [float(s) for s in h["score"]])


def top_results_bubble_sort(indices: List[int], scores: List[float], number_required: int) -> None:
    """fingerprintdb_cuda.cpp:92-103, in place."""
    count = len(indices)
    for i in range(number_required):
        for j in range(count - 1, i, -1):
            if scores[j] > scores[j - 1]:
                indices[j], indices[j - 1] = indices[j - 1], indices[j]
                scores[j], scores[j - 1] = scores[j - 1], scores[j]
