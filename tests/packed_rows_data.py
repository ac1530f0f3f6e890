"""The oracle's packed C3-HLAC rows (test_packed_rows_data_cpu.py, test_gpu_packed_rows.py,
test_gpu_pca_from_clouds.py): the rows with exist > 0 of c3_rows_data.reference, frame after frame
in row order, with their (frame, row, exist) records and the frames' ranges -- what
c3h_extract_c3_frames_packed writes.  The references are c3_rows_data's own, computed once and left
unchanged; nothing here reads a GPU."""
import numpy as np

import c3_rows_data as rd
import c3_sparse_data as sd
from conftest import THR

CASES = {  # name: (clouds, subdivision, offset, thr, packed rows, empty rows) -- the issue's table
    "ladder_a": (lambda: [sd.ladder_a()], sd.LADDER_SUBDIV, (0, 0, 0), sd.LADDER_THR, 13, 1),
    "ladder_a_off": (lambda: [sd.ladder_a()], sd.LADDER_SUBDIV, (0, 1, 0), sd.LADDER_THR, 10, 4),
    "ladder_ba": (lambda: [sd.ladder_b(), sd.ladder_a()], sd.LADDER_SUBDIV, (0, 0, 0), sd.LADDER_THR, 18, 2),
    "ladder_ba_off": (lambda: [sd.ladder_b(), sd.ladder_a()], sd.LADDER_SUBDIV, (0, 1, 0), sd.LADDER_THR, 14, 6),
    "mixed_boxes": (lambda: list(sd.mixed_boxes()), sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, 1067, 69),
    "many_rows": (lambda: [sd.many_rows()], sd.MANY_SUBDIV, (0, 0, 0), THR, 10491, 7059),
}
MIXED_ROWLESS = 12  # frames of mixed_boxes without a row


class Packed:
    pass


def packed(clouds, subdiv, offset, thr, color_mode, variant):
    """rows (n, variant) float32, frame (n,) int32, row (n,) int64, exist (n,) int32, frame_first
    (len(clouds) + 1,) int64 and refs (None for a cloud without a point) of a call."""
    p = Packed()
    p.refs = [rd.reference(c, rd.LEAF, subdiv, offset, thr, color_mode, variant) if len(c) else None for c in clouds]
    rows, frame, row, exist, first = [], [], [], [], [0]
    for k, r in enumerate(p.refs):
        if r is not None and r.hn > 0:
            on = np.flatnonzero(r.ex > 0)
            rows.append(r.fe[on])
            frame.append(np.full(len(on), k, np.int32))
            row.append(on.astype(np.int64))
            exist.append(r.ex[on].astype(np.int32))
        first.append(first[-1] + (len(rows[-1]) if r is not None and r.hn > 0 else 0))
    p.rows = np.concatenate(rows).astype(np.float32) if rows else np.zeros((0, variant), np.float32)
    p.frame = np.concatenate(frame) if frame else np.zeros(0, np.int32)
    p.row = np.concatenate(row) if row else np.zeros(0, np.int64)
    p.exist = np.concatenate(exist) if exist else np.zeros(0, np.int32)
    p.frame_first = np.array(first, np.int64)
    p.n = len(p.rows)
    return p
