"""The bucket cutter and the ready tracking of reducer.GradReducer, without a process group: ``launch``
(the only thing the tracking calls that would issue a collective) is replaced by a recorder."""
import pytest
import torch
import torch.distributed as dist

from sae_vision_amd.reducer import GradReducer, cut_buckets, parse_emulate_rccl

# five parameters of 5, 12, 3, 16 and 7 elements, each start rounded up to 4 elements (train.flat_layout)
SIZES = [5, 12, 3, 16, 7]
OFFS, TOTAL = [0, 8, 20, 24, 40], 48


def _check_cut(ranges, members, cap):
    assert ranges[0][1] == TOTAL and ranges[-1][0] == 0                     # tile [0, TOTAL) from the end
    assert all(ranges[b][0] == ranges[b + 1][1] for b in range(len(ranges) - 1))
    assert all(hi - lo >= cap for lo, hi in ranges[:-1])                     # all but the last one cut
    assert [i for ms in members for i in ms] == list(reversed(range(len(OFFS))))
    assert all(ms and lo == OFFS[ms[-1]] for (lo, _), ms in zip(ranges, members))   # parameter boundaries


def test_cut_buckets_by_hand():
    ranges, members = cut_buckets(OFFS, TOTAL, 16)
    assert ranges == [(24, 48), (8, 24), (0, 8)] and members == [[4, 3], [2, 1], [0]]
    ranges, members = cut_buckets(OFFS, TOTAL, 20)      # (24, 48) holds 24; the rest never reaches 20 again
    assert ranges == [(24, 48), (0, 24)] and members == [[4, 3], [2, 1, 0]]


@pytest.mark.parametrize("cap", [1, 4, 8, 9, 16, 17, 24, 25, 47, 48, 49, 1000])
def test_cut_buckets_tile_from_the_end(cap):
    ranges, members = cut_buckets(OFFS, TOTAL, cap)
    _check_cut(ranges, members, cap)
    if cap > TOTAL:
        assert ranges == [(0, TOTAL)] and members == [[4, 3, 2, 1, 0]]
    if cap == 1:
        assert members == [[4], [3], [2], [1], [0]]
        assert ranges == [(40, 48), (24, 40), (20, 24), (8, 20), (0, 8)]


def _reducer():
    flat = torch.zeros(TOTAL)
    r = GradReducer(flat, OFFS, 16)      # buckets [4, 3], [2, 1], [0]
    rec = []
    r.launch = rec.append
    return r, rec, flat


def test_nothing_launches_outside_a_window():
    r, rec, _ = _reducer()
    for i in range(5):
        r.on_ready(i)
    assert rec == [] and not r.armed


def test_a_bucket_launches_when_its_last_member_reports():
    r, rec, flat = _reducer()
    ptr = lambda i: flat.data_ptr() + 4 * OFFS[i]
    with r.window():
        assert r.armed
        r.on_ready(4)
        r.on_ready(4)                    # twice: counts once
        assert rec == [] and r.remaining == [1, 2, 1]
        r.on_ready(3)
        assert rec == [0]
        r.on_sink(ptr(1))                # the sink listener: by the address of the flat view
        r.on_sink(ptr(1) + 4)            # no parameter starts there: ignored
        r.on_sink(12345)
        assert rec == [0] and r.ready == {4, 3, 1}
        r.on_sink(ptr(2))
        assert rec == [0, 1]
        r.on_ready(3)
        assert rec == [0, 1]
    assert rec == [0, 1, 2] and not r.armed and r.launched == [True] * 3   # the end launched the rest, once


def test_a_window_launches_unreported_buckets_once_each():
    r, rec, _ = _reducer()
    with r.window():
        r.on_ready(2)
        r.on_ready(1)
    assert rec == [1, 0, 2]
    with r.window():                     # the next window starts afresh
        pass
    assert rec == [1, 0, 2, 0, 1, 2]


def test_an_exception_disarms_without_sweeping():
    r, rec, _ = _reducer()
    with pytest.raises(KeyError):
        with r.window():
            r.on_ready(4)
            raise KeyError("backward failed")
    assert rec == [] and not r.armed
    r.on_ready(3)
    assert rec == []


def test_paused_marks_buckets_launched_and_requests_no_collective():
    r, rec, _ = _reducer()
    with r.paused():
        assert not r.enabled
        with r.window():
            r.on_ready(4)
            r.on_ready(3)
            assert r.launched == [True, False, False]
        assert r.launched == [True] * 3
        r.between()
    assert rec == [] and r.enabled
    with pytest.raises(KeyError):
        with r.paused():
            raise KeyError
    assert r.enabled
    assert not dist.is_initialized()     # (a collective would have raised)


@pytest.mark.parametrize("text,want", [("8,300,8", (8, 300.0, 8, 65536, 256)),
                                       ("8,300,8,32", (8, 300.0, 8, 32768, 256)),
                                       ("8,300,8,32,128", (8, 300.0, 8, 32768, 128)),
                                       ("", None)])
def test_parse_emulate_rccl(text, want):
    got = parse_emulate_rccl(text)
    assert got == want and (want is None or [type(x) for x in got] == [int, float, int, int, int])
