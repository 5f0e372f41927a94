"""GPU (MI355X): the stream contract - "asynchronous on `stream`; no allocation, no synchronisation" - of the entry points
of the re-timing of repeated frames (tests/dedup_stream_rows.py), through the instrument of tests/stream_contract.py:
warm up on a side stream, capture one call into a graph, replay it twice on other inputs over poisoned outputs, compare
bit for bit with an eager call on the default stream.  For fiunet_retime_table_* the replay also shows that the host
array of entries is not needed once the call has returned: the row overwrites it right after each call."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_stream_rows as DR  # noqa: E402
import stream_contract as SC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = SC.Env(torch.device("cuda:0"))
    yield e
    e.close()


@pytest.mark.parametrize("row", DR.ROWS, ids=[f"{r.entry}-{r.ident}" for r in DR.ROWS])
def test_captured_replay_equals_the_eager_call(env, row):
    SC.check_row(row, env)
