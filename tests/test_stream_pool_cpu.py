"""CPU tests of the streaming ownership rule (stream.owned_windows: every pooling window of a long record belongs to exactly
one chunk) and of the assembler that puts the chunks' pooled strips and additive sums together (stream.PooledRecord)."""
import numpy as np
import pytest
import torch

from quantum_inferno_amd import engine, stream

KNOWN = [
    # n_total, chunk, hop, factor, edges, offsets edges[i] - starts[i] (None: not recorded)
    (5000, 1024, 512, 24, [0, 768, 1272, 1776, 2304, 2808, 3312, 3840, 4272, 4992], [0, 256, 248, 240, 256, 248, 240, 256, 296]),
    (5000, 1024, 512, 257, [0, 514, 1028, 1542, 2056, 2570, 3084, 3598, 4112, 4883], None),
    (49929, 16384, 8192, 100, [0, 12200, 20400, 28600, 36800, 41300, 49900], None),
    (4096, 1024, 1024, 8, [0, 1024, 2048, 3072, 4096], None),
    (1024, 1024, 512, 8, [0, 1024], None),
]


@pytest.mark.parametrize("n_total,chunk,hop,factor,edges,offsets", KNOWN)
def test_owned_windows_known_answers(n_total, chunk, hop, factor, edges, offsets):
    starts, got = stream.owned_windows(n_total, chunk, hop, factor)
    assert starts.dtype == np.int64 and got.dtype == np.int64
    assert np.array_equal(starts, stream.chunk_starts(n_total, chunk, hop))
    assert got.tolist() == edges
    if offsets is not None:
        assert (got[:-1] - starts).tolist() == offsets


def test_owned_windows_last_offset_is_arbitrary():
    starts, edges = stream.owned_windows(49929, 16384, 8192, 100)
    assert int(edges[-2] - starts[-1]) == 7755


def test_owned_windows_errors():
    with pytest.raises(ValueError, match="24"):
        stream.owned_windows(4096, 1024, 1024, 24)  # hop == chunk and a factor that does not divide the hop
    with pytest.raises(ValueError, match="1"):
        stream.owned_windows(4096, 1024, 512, 1)
    with pytest.raises(ValueError):
        stream.owned_windows(4096, 1024, 512, 0)


def test_owned_windows_partition():
    checked = 0
    for chunk in (1024, 16384):
        for n_total in (chunk, chunk + 1, 3 * chunk + 777, 5000):
            for hop in (chunk // 2, 3 * chunk // 4):
                for factor in (2, 7, 64, 100, 256):
                    where = (n_total, chunk, hop, factor)
                    try:
                        starts, edges = stream.owned_windows(n_total, chunk, hop, factor)
                    except ValueError:
                        continue
                    checked += 1
                    assert len(edges) == len(starts) + 1, where
                    assert np.all(edges % factor == 0) and np.all(np.diff(edges) >= 0), where
                    assert edges[0] == 0 and edges[-1] == n_total // factor * factor, where
                    assert np.all(edges[:-1] >= starts) and np.all(edges[1:] <= starts + chunk), where
                    # the windows of the chunks, one after the other, are the windows of the record: each exactly once
                    first = edges[:-1] // factor
                    count = np.diff(edges) // factor
                    assert first[0] == 0 and np.array_equal(first[1:], np.cumsum(count)[:-1]) and count.sum() == n_total // factor, where
    assert checked == 70  # (refused: only the 10 cases of a 5000-sample record and 16384-sample chunks)


def _item(index, c0, cb, w0, nw, bands, seed, methods):
    g = torch.Generator().manual_seed(seed)
    strips = {m: torch.rand((cb, bands, nw), generator=g) for m in methods}
    band = torch.rand((cb, bands), generator=g, dtype=torch.float64)
    stats = torch.rand((cb, 4), generator=g, dtype=torch.float64)
    res = engine.TfrResult(frequency_hz=np.arange(1.0, bands + 1), power_band=band, stats=stats, power_scale=2.0, pooled=strips)
    return stream.StreamItem(index, c0, cb, index, 0, res, None, w0, nw)


def test_pooled_record_places_and_adds():
    methods = ("average", "max")
    rec = stream.PooledRecord(3, 5, 10, methods, torch.float32, "cpu")
    assert all(tuple(rec.panel[m].shape) == (3, 5, 10) and bool(torch.isnan(rec.panel[m]).all()) for m in methods)
    a = _item(0, 1, 2, 0, 4, 5, 11, methods)
    b = _item(1, 1, 2, 4, 6, 5, 12, methods)
    rec.add(a, "cwt")
    rec.add(b, "cwt")
    for m in methods:
        assert torch.equal(rec.panel[m][1:3, :, :4], a.cwt.pooled[m]) and torch.equal(rec.panel[m][1:3, :, 4:], b.cwt.pooled[m])
        assert bool(torch.isnan(rec.panel[m][0]).all())  # nobody added channel 0
    out = rec.result()
    assert out.pooled is rec.panel and out.power_time is None and out.power_scale == 2.0
    assert torch.equal(out.power_band[1:3], a.cwt.power_band + b.cwt.power_band) and bool((out.power_band[0] == 0).all())
    assert torch.equal(out.stats[1:3, 1:3], a.cwt.stats[:, 1:3] + b.cwt.stats[:, 1:3])
    assert torch.equal(out.stats[1:3, 0], torch.maximum(a.cwt.stats[:, 0], b.cwt.stats[:, 0]))
    assert torch.equal(out.total_power[1:3], (a.cwt.stats + b.cwt.stats)[:, 1])
    assert np.array_equal(out.frequency_hz, a.cwt.frequency_hz)
    with pytest.raises(ValueError):
        rec.add(a, "stx")  # the item carries no Stockwell strips


def test_stream_item_and_result_defaults():
    item = stream.StreamItem(0, 0, 1, 0, 0, None, None)
    assert item.window0 is None and item.windows is None
    assert engine.TfrResult(frequency_hz=np.zeros(1)).pooled is None
