"""ppk_strain_extend_dev (include/ppk.h "Lineages within every strain") restated in numpy, strain by
strain, through the steps a caller takes without it: cut the strain's query square and query x reference rectangle out
of the two matrices, floor them, oracle.extend on the strain's stored triplets; then lineage_model.strain_ranks
(oracle.lower_rank per rank, components, printClusters' numbering) over the extended segments.  (oracle.extend and
oracle.lower_rank are restatements by reading: parity with the reference's C++ is unpinned, see oracle/oracle.py.)"""
import numpy as np

import lineage_model
from oracle import oracle


def stored_offsets(seg_off, depth):
    sizes = np.diff(np.asarray(seg_off, dtype=np.int64))
    return np.concatenate([[0], np.cumsum(sizes * np.minimum(int(depth), sizes - 1))]).astype(np.int64)


def strain_inputs(s, members, seg_off, queries, qry_off, stored, qr, qq, n_ref, n_qry, depth, col, floor):
    """What ppk_extend takes for strain s alone: its stored triplets, its floored query square [q_s, q_s] and its floored
    rectangle [n_s, q_s]."""
    mem = np.asarray(members[seg_off[s]:seg_off[s + 1]], dtype=np.int64)
    qry = np.asarray(queries[qry_off[s]:qry_off[s + 1]], dtype=np.int64)
    nn_off = stored_offsets(seg_off, depth)
    trip = tuple(a[nn_off[s]:nn_off[s + 1]] for a in stored)
    floor = np.float32(floor)
    rect = np.zeros((len(mem), len(qry)), dtype=np.float32)
    square = np.zeros((len(qry), len(qry)), dtype=np.float32)
    if len(qry):
        rect = np.asarray(qr, dtype=np.float32)[qry[None, :] * np.int64(n_ref) + mem[:, None], col]
        lo, hi = np.minimum(qry[:, None], qry[None, :]), np.maximum(qry[:, None], qry[None, :])
        off = np.where(lo != hi, lo * (2 * n_qry - lo - 1) // 2 + (hi - lo - 1), 0)
        if len(qry) > 1:
            square = np.where(lo != hi, np.asarray(qq, dtype=np.float32)[off, col], np.float32(0.0)).astype(np.float32)
    rect = np.where(rect < floor, floor, rect).astype(np.float32)
    square = np.where(square < floor, floor, square).astype(np.float32)
    return trip, np.ascontiguousarray(square), np.ascontiguousarray(rect)


def strain_extend(members, seg_off, queries, qry_off, stored, qr, qq, n_ref, n_qry, depth, col=0, floor=1e-10):
    """(i, j, dist) with local indices over the n_s + q_s rows of every strain; -0.0 comes back as 0.0."""
    oi, oj, od = [], [], []
    for s in range(len(seg_off) - 1):
        trip, square, rect = strain_inputs(s, members, seg_off, queries, qry_off, stored, qr, qq, n_ref, n_qry, depth,
                                           col, floor)
        i, j, d = oracle.extend(trip[0], trip[1], trip[2], square, rect, depth)
        oi.append(i)
        oj.append(j)
        od.append(d + np.float32(0.0))
    return np.concatenate(oi), np.concatenate(oj), np.concatenate(od).astype(np.float32)


def extended_segments(seg_off, qry_off):
    return (np.asarray(seg_off, dtype=np.int64) + np.asarray(qry_off, dtype=np.int64)).astype(np.int64)


def strain_extend_ranks(lists, seg_off, qry_off, depth, ranks, reciprocal_only=False, count_unique_distances=False,
                        epsilon=1e-10):
    """lineage_model.strain_ranks over the extended segments: oracle.lower_rank sorts every row stably by distance, which
    leaves extend's order inside a run of equal distances as it is."""
    return lineage_model.strain_ranks(lists, extended_segments(seg_off, qry_off), depth, ranks, reciprocal_only,
                                      count_unique_distances, epsilon)
