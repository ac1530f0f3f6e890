"""The clouds of c3_sparse_data.py without a GPU: the oracle and numpy alone show that every shape
test_gpu_c3_sparse.py is written for is in its inputs -- group lengths at the chunk and slice
edges, group heads and ends on the plan tile's edges, a last group at vtot with and without "none"
keys behind it, more rows and chunks than one launch holds, non-cubic and tiny frames, voxels
whose centroid lies in another cell with each of their interactions.  These are conditions on the
inputs, not tolerances.

Two conditions are other than first planned, both because no cloud can meet them.  A row of one
voxel (many_rows at subdivision 1) fills at most 618 of the 981 bins: 6 + 468 + 21 of the colour
half, and of the binarised half the 3 of 6 centre bins that are set, their 9 products per
neighbour (117) and 3 of the 12 channel pairs; the cloud must reach exactly that.  And
test_gpu_points_exact.py has no `_stats`: its _moved_list, _interactions and
_assert_batched_frame are used."""
import numpy as np
import pytest

import c3_sparse_data as sd
import convosch_data as cd
import test_gpu_points_exact as tpe
from conftest import THR

T, C, S = sd.PLAN_TILE, sd.CHUNK, sd.SLICE
ARRANGEMENTS = {"A": ("a",), "AB": ("a", "b"), "BA": ("b", "a")}
ONE_VOXEL_BINS = 6 + 468 + 21 + 3 + 117 + 3


def _ladder(name):
    return sd.ladder_a() if name == "a" else sd.ladder_b()


def _ladder_refs(arr, offset, cm=sd.CM):
    return [sd.reference(_ladder(n), sd.LEAF, sd.LADDER_SUBDIV, offset, sd.LADDER_THR, cm) for n in ARRANGEMENTS[arr]]


def _filled(r):
    """The largest number of non-zero bins among the rows that exist."""
    return int((r.fe[r.ex > 0] != 0).sum(1).max())


def test_ladder_rows_hold_the_stated_voxels():
    for cm in sd.COLOR_MODES:
        a = sd.reference(sd.ladder_a(), sd.LEAF, sd.LADDER_SUBDIV, (0, 0, 0), sd.LADDER_THR, cm)
        assert a.div_b == (174, 13, 13) and a.n_occ == 11_655 and a.n_moved == 0
        assert a.sb == (14, 1, 1) and a.hn == 14
        counts, none = sd.row_counts(a, sd.LADDER_SUBDIV, (0, 0, 0))
        assert counts.tolist() == list(sd.LADDER_A) and none == 0
        assert a.ex[6] == 0 and (np.delete(a.ex, 6) > 0).all()  # an empty row between full ones
        b = sd.reference(sd.ladder_b(), sd.LEAF, sd.LADDER_SUBDIV, (0, 0, 0), sd.LADDER_THR, cm)
        assert b.n_occ == 2 * C == T and b.n_moved == 0 and b.hn == len(sd.LADDER_B)
        assert sd.row_counts(b, sd.LADDER_SUBDIV, (0, 0, 0))[0].tolist() == list(sd.LADDER_B) and sd.LADDER_B[-1] == 1
        assert b.ex[2] == 0 and (np.delete(b.ex, 2) > 0).all()
        assert _filled(a) == 981 and _filled(b) == 981
    # at offset (0, 1, 0) the cells of y = 0 feed no row: rows 1, 11 and 13 of A lose every voxel
    a = _ladder_refs("A", (0, 1, 0))[0]
    counts, none = sd.row_counts(a, sd.LADDER_SUBDIV, (0, 1, 0))
    assert a.hn == 14 and [i for i in range(14) if counts[i] == 0] == [1, 6, 11, 13] and none == 987
    assert (a.ex[[1, 6, 11, 13]] == 0).all() and (np.delete(a.ex, [1, 6, 11, 13]) > 0).all()


def test_ladder_colours_sit_on_the_thresholds():
    for pts in (sd.ladder_a(), sd.ladder_b()):
        word = pts[:, 3].view(np.uint32)
        for ch, thr in zip((16, 8, 0), sd.LADDER_THR):
            v = (word >> ch) & 255
            for want in (0, thr - 1, thr, thr + 1, 254, 255):
                assert (v == want).sum() >= 20, (ch, want)
    assert len(set(sd.LADDER_THR)) == 3  # a swap of two channels' thresholds moves voxels across them


@pytest.mark.parametrize("offset", sd.LADDER_OFFSETS)
def test_ladder_group_lengths(offset):
    """Every chunk and slice edge is the length of some group, at either offset."""
    lens = set()
    for arr in ARRANGEMENTS:
        groups, vtot, none = sd.batch_positions(_ladder_refs(arr, offset), sd.LADDER_SUBDIV, offset)
        lens |= {n for _, n in groups}
    if offset == (0, 0, 0):
        for name, n in (("one voxel", 1), ("a slice less one", S - 1), ("one slice", S), ("a slice and one", S + 1),
                        ("a chunk less one", C - 1), ("one full chunk", C), ("a chunk and one voxel", C + 1),
                        ("two chunks less one", 2 * C - 1), ("two full chunks", 2 * C), ("two chunks and one", 2 * C + 1)):
            assert n in lens, name
    else:  # the shorter groups of the none-key variant: still several chunks, single chunks, part slices
        assert any(n > C for n in lens) and any(S < n < C for n in lens) and any(n < S for n in lens)


def test_ladder_plan_tile_conditions():
    """Per arrangement and offset the groups' sorted positions; each condition holds where stated."""
    seen = {}
    for arr in ARRANGEMENTS:
        for offset in sd.LADDER_OFFSETS:
            groups, vtot, none = sd.batch_positions(_ladder_refs(arr, offset), sd.LADDER_SUBDIV, offset)
            last = groups[-1]
            seen[arr, offset] = dict(
                head_on_tile_end=any(p % T == T - 1 and n >= 2 for p, n in groups),  # its gallop reads the next tile
                head_on_tile_start=any(p % T == 0 and p > 0 for p, n in groups),
                end_on_tile_end=any((p + n - 1) % T == T - 1 for p, n in groups),
                second_chunk_on_tile_start=any(n > C and (p + C) % T == 0 for p, n in groups),
                one_voxel_on_tile_end=any(p % T == T - 1 and n == 1 for p, n in groups),
                last_of_one_at_vtot=last == (vtot - 1, 1) and none == 0,
                last_of_five_at_vtot=last == (vtot - 5, 5) and none == 0,
                none_keys_behind=none > 0 and last[0] + last[1] == vtot - none,
                tiles=-(-vtot // T))
    zero = (0, 0, 0)
    # A alone and [A, B] keep A's positions; [B, A] moves them by B's 2,048 voxels, one whole tile
    for arr in ("A", "AB", "BA"):
        s = seen[arr, zero]
        assert s["head_on_tile_end"] and s["head_on_tile_start"] and s["end_on_tile_end"], arr
        assert s["second_chunk_on_tile_start"], arr
    assert seen["BA", zero]["one_voxel_on_tile_end"]  # B's last group on 2047, A's first head on 2048
    assert seen["AB", zero]["last_of_one_at_vtot"]  # the head is position vtot - 1
    assert seen["A", zero]["last_of_five_at_vtot"] and seen["BA", zero]["last_of_five_at_vtot"]  # the gallop overshoots vtot
    for arr in ARRANGEMENTS:
        assert seen[arr, (0, 1, 0)]["none_keys_behind"], arr
    assert seen["AB", zero]["tiles"] == 7 and seen["A", zero]["tiles"] == 6  # several tiles, the last one part full


def test_many_rows_pass_both_launch_bounds():
    r = sd.reference(sd.many_rows(), sd.LEAF, sd.MANY_SUBDIV, (0, 0, 0), THR, sd.CM)
    counts, none = sd.row_counts(r, sd.MANY_SUBDIV, (0, 0, 0))
    assert r.div_b == (27, 26, 25) and r.hn == 17_550 > 16_384 and r.n_moved == 0 and none == 0
    assert set(counts.tolist()) == {0, 1} and (counts == 1).sum() == r.n_occ == 10_491 > 4_096 + 4_096
    assert (r.ex > 0).sum() == 10_491 and (counts == 0).sum() == 7_059
    # beyond the first trip of either loop: rows and chunks past the launch's last workgroup
    assert (r.ex[16_384:] > 0).any() and (r.ex[16_384:] == 0).any()
    assert _filled(r) == ONE_VOXEL_BINS  # what a row of one voxel can fill (module docstring)
    # the frames around it in the batch: LADDER_B has rows at this subdivision too
    b = sd.reference(sd.ladder_b(), sd.LEAF, sd.MANY_SUBDIV, (0, 0, 0), THR, sd.CM)
    assert 0 < b.hn < r.hn and (b.ex > 0).sum() == 2048


def test_mixed_boxes_are_non_cubic_tiny_and_rowless():
    refs = [sd.reference(p, sd.LEAF, sd.MIXED_SUBDIV, sd.MIXED_OFFSET, THR, sd.CM) for p in sd.mixed_boxes()]
    assert len(refs) == 64 and all(r.hn >= 0 for r in refs)
    assert sum(len(set(r.div_b)) == 3 for r in refs) >= 8  # three different extents
    assert len({r.div_b for r in refs}) >= 50 and len({r.min_b for r in refs}) >= 50
    assert sum(r.hn == 0 for r in refs) >= 3  # no row: an offset reaches the grid's end
    assert sum(r.n_occ <= 2 for r in refs) >= 3
    assert [refs[k].n_occ for k in sd.ONE_CELL] == [1, 1, 1] and all(refs[k].div_b == (1, 1, 1) for k in sd.ONE_CELL)
    assert [refs[k].n_occ for k in sd.TWO_VOXELS] == [2, 2, 2] and all(refs[k].hn > 0 for k in sd.TWO_VOXELS)
    assert sum(r.hn > 0 and (r.ex > 0).any() for r in refs) >= 30
    assert sum(r.hn > 0 and (r.ex == 0).any() for r in refs) >= 3  # rows that stay zero among them
    # a swap of div_b[0] and div_b[1] in a linear index shows only where they differ and both exceed 1
    assert sum(r.div_b[0] != r.div_b[1] and min(r.div_b[:2]) > 1 and r.hn > 0 for r in refs) >= 30
    assert max(_filled(r) for r in refs if r.hn > 0 and (r.ex > 0).any()) == 981
    assert all(r.n_moved == 0 for r in refs)


def test_face_frames_move_voxels_in_every_way():
    frames = sd.face_frames()
    assert set(frames) == {(6, (0, 0, 0)), (5, (2, 1, 0)), (16, (0, 0, 0)), (0, (0, 0, 0))}
    total = dict(multi=0, onto=0, pairs=0, cross=0, into_empty=0, single_out=0, below_zero=0)
    for (sub, off), batch in frames.items():
        rows = []
        for name, pts, own in batch:
            r = sd.reference(pts, sd.LEAF, sub, off, THR, sd.CM)
            assert r.hn > 0, (name, sub, off, r.hn)  # no centroid past the last subdivision (-5)
            assert 20 <= r.n_moved <= 256, (name, r.n_moved)
            assert _filled(r) >= 900, (name, _filled(r))
            rows.append(r.hn)
            if not own:
                continue
            t = tpe._reference(pts, 981, sub, off, sd.CM)  # the moved list and the uncorrected rows
            assert t.n_moved == r.n_moved == int(tpe._moved_list(r.g, r.layout, r.cloud)[2].sum())
            assert np.array_equal(t.fe, r.fe) and t.sb == r.sb
            tpe._assert_batched_frame(pts, t, sub, off)  # rows differ: >= 10, or the one row; the by-hand voxels
            several = tpe._several(sub, off, min(r.div_b))
            assert t.rows_differ >= (10 if several else 1) and several == (r.hn > 1)
            multi, onto, pairs, cross, into_empty, single_out = tpe._interactions(t, sub, off)
            below = int((t.moved & (t.own[:, 0] == 0) & (t.cc[:, 0] == -1)).sum())
            for k, v in zip(total, (multi, onto, pairs, cross, into_empty, single_out, below)):
                total[k] += v
            assert below >= 1, name  # a voxel in cell 0 of x whose centroid cell is -1
        # the one-subdivision frame stands in a batch with frames of several rows
        if sub == 16:
            assert rows[0] == 1 and max(rows) > 1
        if sub == 0:
            assert rows == [1] * len(rows) and max(sd.reference(p, sd.LEAF, sub, off, THR, sd.CM).n_occ for _, p, _ in batch) > 3 * C
    # every interaction of test_gpu_points_exact.py's docstring, by name
    for k, v in total.items():
        assert v >= 1, k


def test_white_plane_and_ladder_in_groups_of_several_chunks():
    """The first call of the one-context test: at subdivision 50 the plane's 36 rows hold 2,500
    voxels each, so that call has the most groups of several chunks."""
    multi = {}
    for name, clouds, sub, off in (("first", [cd.white_plane(), sd.ladder_a()], 50, (0, 0, 0)),
                                   ("mixed", list(sd.mixed_boxes()), sd.MIXED_SUBDIV, sd.MIXED_OFFSET),
                                   ("ladder", [sd.ladder_a()], sd.LADDER_SUBDIV, (0, 0, 0)),
                                   ("many", [sd.many_rows()], sd.MANY_SUBDIV, (0, 0, 0))):
        refs = [sd.reference(p, sd.LEAF, sub, off, sd.LADDER_THR if name in ("first", "ladder") else THR, sd.CM) for p in clouds]
        groups, vtot, none = sd.batch_positions(refs, sub, off)
        multi[name] = sum(n > C for _, n in groups)
    assert multi == {"first": 36 + 3, "mixed": 0, "ladder": 5, "many": 0}, multi
