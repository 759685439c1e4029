"""CPU tests of the pure-Python job builders of hipblosc.py -- region_jobs, slice_jobs, index_jobs: what CBloscReadRegion, CBloscReadSlices and
CBloscReadOIndex cut a selection of a chunked array into.  Every job is applied here with plain numpy indexing -- its selection of its chunk's
array, into the output at the job's offset and strides -- and the assembled output has to be what numpy gives for the whole array.  No library
and no device: the jobs are ctypes records."""
import numpy as np
import pytest

import hipblosc as hb

PAD = -1                             # what a chunk at the array's edge holds beyond the array: no job may select it
# (array shape, chunk shape): the last chunk of every dimension is ragged
ARRAYS = {2: ((10, 7), (4, 3)), 3: ((5, 7, 9), (2, 3, 4))}


def _chunked(nd):
    """the array, its chunk grid, the chunk shape and the chunks in C order of the grid, each stored whole"""
    shape, chunk = ARRAYS[nd]
    z = np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape)
    grid = tuple(-(-a // c) for a, c in zip(shape, chunk))
    padded = np.full([g * c for g, c in zip(grid, chunk)], PAD, np.int32)
    padded[tuple(slice(0, a) for a in shape)] = z
    chunks = [padded[tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, chunk))] for idx in np.ndindex(*grid)]
    return z, grid, chunk, chunks


def _assemble(pairs, out_shape, chunks, chunk, pick):
    """the output of the jobs `pairs`: pick(job, chunk array) is the job's selection, placed at the job's offset with the job's strides"""
    out = np.full(int(np.prod(out_shape)) * 4, 0xEE, np.uint8)
    written = np.zeros(out.size, bool)
    for job, off in pairs:
        nd = job.ndim
        assert 0 <= job.frame < len(chunks) and tuple(job.chunk_shape[:nd]) == tuple(chunk)
        got = pick(job, chunks[job.frame])
        assert off % 4 == 0 and all(s % 4 == 0 for s in job.dst_stride[:nd]) and got.size > 0
        reach = off + sum((m - 1) * s for m, s in zip(got.shape, job.dst_stride[:nd])) + 4
        assert reach <= out.size, "a job writes beyond the output"
        np.lib.stride_tricks.as_strided(out[off:].view(np.int32), got.shape, tuple(job.dst_stride[:nd]))[...] = got
        np.lib.stride_tricks.as_strided(written[off:].view(np.uint8).view(np.int32), got.shape, tuple(job.dst_stride[:nd]))[...] = 0x01010101
    assert written.all(), "the jobs leave a part of the output unwritten"
    return out.view(np.int32).reshape(out_shape)


def _pick_box(job, c):
    return c[tuple(slice(job.start[k], job.start[k] + job.shape[k]) for k in range(job.ndim))]


def _pick_slice(job, c):
    return c[tuple(slice(job.start[k], job.start[k] + (job.count[k] - 1) * job.step[k] + 1, job.step[k]) for k in range(job.ndim))]


def _pick_index(index):
    def pick(job, c):
        sel = []
        for k in range(job.ndim):
            if job.list[k] < 0:
                sel.append(job.start[k] + np.arange(job.count[k]) * job.step[k])
            else:
                sel.append(np.array(index[job.list[k]: job.list[k] + job.count[k]], np.int64))
            assert sel[-1].size == job.count[k] and (sel[-1] >= 0).all() and (sel[-1] < job.chunk_shape[k]).all()
        return c[np.ix_(*sel)]
    return pick


REGIONS = {2: [[(0, 10), (0, 7)], [(3, 9), (2, 7)], [(4, 8), (3, 6)], [(9, 10), (6, 7)], [(5, 6), (0, 7)], [(2, 2), (1, 5)], [(0, 10), (7, 7)]],
           3: [[(0, 5), (0, 7), (0, 9)], [(1, 4), (2, 7), (3, 8)], [(4, 5), (6, 7), (8, 9)], [(2, 4), (3, 6), (4, 8)], [(0, 5), (3, 3), (0, 9)]]}


@pytest.mark.parametrize("nd", [2, 3])
def test_region_jobs_assemble_the_numpy_slice(nd):
    z, grid, chunk, chunks = _chunked(nd)
    for region in REGIONS[nd]:
        pairs, out_shape = hb.region_jobs(grid, chunk, region, 4)
        want = z[tuple(slice(lo, hi) for lo, hi in region)]
        assert tuple(out_shape) == want.shape
        if want.size == 0:
            assert pairs == []
            continue
        spans = [(hi - 1) // c - lo // c + 1 for (lo, hi), c in zip(region, chunk)]
        assert len(pairs) == int(np.prod(spans)), "one job per chunk the region crosses"
        assert np.array_equal(_assemble(pairs, out_shape, chunks, chunk, _pick_box), want), region


# (lo, hi, step): whole, odd steps, a step that jumps a whole chunk (and with it whole rows of the grid), one item, nothing
SLICES = {2: [[(0, 10, 1), (0, 7, 1)], [(1, 10, 3), (0, 7, 2)], [(0, 10, 9), (1, 7, 5)], [(2, 10, 5), (0, 7, 4)], [(7, 8, 1), (4, 5, 3)], [(3, 3, 2), (0, 7, 1)]],
          3: [[(0, 5, 1), (0, 7, 1), (0, 9, 1)], [(1, 5, 2), (0, 7, 3), (2, 9, 5)], [(0, 5, 4), (1, 7, 5), (0, 9, 7)], [(4, 5, 1), (6, 7, 1), (8, 9, 1)],
              [(0, 5, 1), (0, 7, 2), (5, 5, 1)]]}


@pytest.mark.parametrize("nd", [2, 3])
def test_slice_jobs_assemble_the_numpy_stepped_slice(nd):
    z, grid, chunk, chunks = _chunked(nd)
    for slices in SLICES[nd]:
        pairs, out_shape = hb.slice_jobs(grid, chunk, slices, 4)
        want = z[tuple(slice(lo, hi, st) for lo, hi, st in slices)]
        assert tuple(out_shape) == want.shape
        if want.size == 0:
            assert pairs == []
            continue
        held = [len({i // c for i in range(lo, hi, st)}) for (lo, hi, st), c in zip(slices, chunk)]
        assert len(pairs) == int(np.prod(held)), "one job per chunk that holds a selected item: a chunk a step jumps over gets none"
        assert np.array_equal(_assemble(pairs, out_shape, chunks, chunk, _pick_slice), want), slices


# per dimension a (lo, hi, step) triple or a list: unsorted with repeats, sorted, one index, none
OINDEX = {2: [[[9, 0, 4, 4, 3, 8, 0], [6, 2, 2, 5, 0]], [(1, 10, 3), [5, 1, 6, 1]], [[2, 7, 3], (0, 7, 5)], [[0, 1, 2, 3, 4, 5], [0, 3, 6]], [[8], [6]], [[], [1, 2]],
              [(0, 10, 9), [3, 3]]],
          3: [[[4, 0, 2, 2], [6, 1, 3, 3, 0], [8, 0, 4, 5, 3, 3]], [(0, 5, 2), [5, 2], (1, 9, 7)], [[3], (6, 7, 1), [8]], [[1, 4], [], (0, 9, 1)],
              [(0, 5, 4), (0, 7, 6), [7, 0, 8, 4]]]}


@pytest.mark.parametrize("nd", [2, 3])
def test_index_jobs_assemble_the_numpy_orthogonal_selection(nd):
    z, grid, chunk, chunks = _chunked(nd)
    for selection in OINDEX[nd]:
        pairs, index, out_shape = hb.index_jobs(grid, chunk, selection, 4)
        want = z[np.ix_(*[np.arange(*s) if isinstance(s, tuple) else np.array(s, np.int64) for s in selection])]
        assert tuple(out_shape) == want.shape
        if want.size == 0:
            assert pairs == []
            continue
        assert np.array_equal(_assemble(pairs, out_shape, chunks, chunk, _pick_index(index)), want), selection
