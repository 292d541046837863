"""vbz_gpu_events_query_batch on the MI355X, bit for bit against eventalign_ref's numpy statement, canary words around every arena: rows
per read on both sides of a 64-row turn, every N, kept counts around N, drops at a turn's seam, means copied bitwise, verdicts, the bad
shapes of event_first beside good reads, index NULL, thousands of one-row reads, and GpuCodec.events_query."""
import re

import numpy as np
import pytest
import torch

import eventalign_ref as E
from eventalign_support import assert_query, dev_u32, dev_u64, records_of, stage_query
from typed_support import codec

pytestmark = pytest.mark.gpu

COUNTS, TABLES = E.query_counts(), E.query_tables()


def _ids(calls):
    return [re.sub(r"[^A-Za-z0-9]+", "-", c.name)[:60] for c in calls]


@pytest.mark.parametrize("call", COUNTS, ids=_ids(COUNTS))
def test_rows_and_kept_counts(call):
    want = call.expected()
    assert_query(stage_query(codec(), call), want, call)


@pytest.mark.parametrize("call", TABLES, ids=_ids(TABLES))
def test_tables(call):
    want = call.expected()
    got = stage_query(codec(), call)
    assert (got[2] is None) == (not call.use_index)
    assert_query(got, want, call)


def test_the_python_method():
    c = codec()
    call = [t for t in TABLES if t.name == "an error verdict"][0]
    want = call.expected()
    first, rec, res = dev_u64(c, call.first), records_of(c, call.mean, call.n).reshape(-1, 4), dev_u32(c, call.result)
    query, valid, index = c.events_query(first, rec, call.N, min_n=call.min_n, result=res)
    c.synchronize()
    assert query.dtype == torch.float32 and tuple(query.shape) == (4, call.N) and tuple(index.shape) == (4, call.N)
    assert_query((query.cpu().numpy().view(np.uint32), valid.cpu().numpy().view(np.uint32), index.cpu().numpy().view(np.uint32)), want, call)
    out = torch.zeros((4, call.N), dtype=torch.float32, device=c.device)
    q2, v2, i2 = c.events_query(first, rec, call.N, min_n=call.min_n, index=False, query=out)
    c.synchronize()
    assert i2 is None and q2 is out
    want2 = E.events_query(call.first, call.event_rows, call.mean, call.n, call.N, call.min_n)
    assert (out.cpu().numpy().view(np.uint32) == want2[0]).all() and (v2.cpu().numpy().view(np.uint32) == want2[1]).all()
