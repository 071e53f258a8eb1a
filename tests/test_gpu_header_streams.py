"""The entry points of the array headers (include/qi_array.h ... qi_lags.h) order their work on the caller's stream (-m gpu):
every case of the headers' tables (stream_order.TABLES but the first, which tests/test_gpu_streams.py runs with the harness's
positive control) behind the delayed producer of tests/stream_order.py.  Per case: the result equals the serial result on B
bit for bit, differs from the stale result on A as the table's power rule says, the serial outputs pass the table's checks,
and the call returned before its input was written: none of these headers has an entry point that waits on the host."""
import pytest
import torch

import stream_order as so

pytestmark = pytest.mark.gpu

CASES = [(table, cid) for table in so.TABLES[1:] for cid in table.ids()]


@pytest.fixture(scope="module", autouse=True)
def _log():
    yield
    torch.cuda.synchronize()
    so.write_log()


@pytest.mark.parametrize("table,cid", CASES, ids=[f"{table.name}/{cid}" for table, cid in CASES])
def test_ordered_behind_a_delayed_producer(table, cid):
    assert table.by_id(cid).asynchronous
    so.ordered_behind_producer(table, cid)
