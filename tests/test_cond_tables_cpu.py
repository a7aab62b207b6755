"""The scheduler of the AdaRMSNorm scale tables (models/cond_tables.py) under recording fakes, WITHOUT a GPU: which table a call reads,
what fills it, on which stream, and which event each stream waits for first.  Every case states the exact trace of stream operations:
("wait", stream, event), ("record", event, stream), ("fill", chain, stream, repeat), ("run", chain, table address, stream)."""
import contextlib
from importlib import import_module

import pytest
import torch

B, WIDTH = 2, 8


class Stream:
    def __init__(self, trace, name):
        self.trace, self.name = trace, name

    def wait_event(self, event):
        self.trace.append(("wait", self, event))

    def __repr__(self):
        return f"<stream {self.name}>"


class Event:
    def __init__(self, trace, name):
        self.trace, self.name, self.complete, self.queries = trace, name, False, 0

    def record(self, stream):
        self.trace.append(("record", self, stream))

    def query(self):
        self.queries += 1
        return self.complete

    def __repr__(self):
        return f"<event {self.name}>"


class Seam:
    """The stream seam of ScaleTables: one trace, a settable current stream, events numbered in the order they were made."""

    def __init__(self):
        self.trace, self.events, self.is_capturing = [], [], False
        self.main = self.cur = Stream(self.trace, "main")

    def current(self):
        return self.cur

    def side(self, device):
        self.side_stream = Stream(self.trace, "side")
        return self.side_stream

    def event(self):
        self.events.append(Event(self.trace, len(self.events)))
        return self.events[-1]

    @contextlib.contextmanager
    def on(self, stream):
        old, self.cur = self.cur, stream
        try:
            yield
        finally:
            self.cur = old

    def handle(self, stream):
        return stream

    def capturing(self):
        return self.is_capturing

    def take(self):
        out = list(self.trace)
        del self.trace[:]
        return out


class Chain:
    def __init__(self, seam, rows):
        self.seam, self.rows = seam, rows

    def fill(self, sigma, aug_cond, class_cond, mapping_cond, repeat=1):
        self.seam.trace.append(("fill", self, self.seam.cur, repeat))       # (the copies go to the stream that is current)

    def run(self, table_ptr, stream):
        self.seam.trace.append(("run", self, table_ptr, stream))

    def __repr__(self):
        return f"<chain {self.rows}>"


@pytest.fixture
def ct(KD):
    return import_module(KD.__name__ + ".models.cond_tables")


@pytest.fixture
def rig(ct):
    """(tables, seam, chains built so far); the construction itself (side stream, main_entry, the per-step chain) leaves no trace."""
    seam, built = Seam(), []

    def build_chain(rows):
        built.append(Chain(seam, rows))
        return built[-1]
    tables = ct.ScaleTables(B, WIDTH, "cpu", build_chain, streams=seam)
    assert seam.trace == [] and [c.rows for c in built] == [B] and tables.step_chain is built[0]
    assert tables.main_entry is seam.events[0] and tables.side_stream is seam.side_stream
    return tables, seam, built


def sigmas(*values):
    return [torch.full([B], float(v)) for v in values]


def call(tables, sigma, cls):
    """What a model call does: the table, then the mark in front of its main chain."""
    addr = tables.table_for(sigma, None, cls, None)
    tables.mark_entry()
    return addr


def inline(tables, seam, buf, stream=None):
    """Trace of a per-step chain run inline into table ``buf`` (without waits), with the main_entry mark behind it."""
    s = stream or seam.main
    return [("fill", tables.step_chain, s, 1), ("run", tables.step_chain, tables.scales[buf].data_ptr(), s), ("record", tables.main_entry, s)]


def test_plain_calls_alternate_the_tables(rig):
    tables, seam, _ = rig
    cls = torch.tensor([3, 7])
    assert tables.scales[0].shape == (B, WIDTH) and tables.scales[0].data_ptr() != tables.scales[1].data_ptr()
    for sigma, buf in zip(sigmas(5, 4, 3), (0, 1, 0)):
        assert call(tables, sigma, cls) == tables.scales[buf].data_ptr()
        assert seam.take() == inline(tables, seam, buf)                     # fill, run, main_entry: nothing is waited for
        assert tables.last_buf == buf


def test_a_followed_hint_costs_the_call_one_wait(rig):
    tables, seam, _ = rig
    cls = torch.tensor([3, 7])
    s0, s1, s2 = sigmas(5, 4, 3)
    call(tables, s0, cls)                                                   # table 0
    seam.take()
    tables.hint_next(s1, None, cls, None)
    side, done = seam.side_stream, seam.events[-1]
    assert done is not tables.main_entry and len(seam.events) == 2
    assert seam.take() == [("wait", side, tables.main_entry), ("fill", tables.step_chain, side, 1),
                           ("run", tables.step_chain, tables.scales[1].data_ptr(), side), ("record", done, side)]
    assert seam.cur is seam.main                                            # (the side stream was current for the chain only)
    tables.hint_next(s2, None, cls, None)                                   # one is pending: nothing happens
    assert seam.take() == [] and len(seam.events) == 2
    assert tables.pending[0].tensors[0] is s1                               # the record keeps the hinted tensors alive
    assert call(tables, s1, cls) == tables.scales[1].data_ptr()
    assert seam.take() == [("wait", seam.main, done), ("record", tables.main_entry, seam.main)]
    assert tables.pending is None and tables.last_buf == 1


@pytest.mark.parametrize("what", ["sigma", "class"])
def test_an_unused_hint_is_waited_for_and_its_table_rewritten(rig, what):
    tables, seam, _ = rig
    cls = torch.tensor([3, 7])
    s0, s1, s2 = sigmas(5, 4, 3)
    call(tables, s0, cls)
    tables.hint_next(s1, None, cls, None)                                   # into table 1
    done = seam.events[-1]
    seam.take()
    args = (s2, cls) if what == "sigma" else (s1, torch.tensor([3, 8]))
    assert call(tables, *args) == tables.scales[1].data_ptr()               # the buffer the hint wrote, behind the hint
    assert seam.take() == [("wait", seam.main, done)] + inline(tables, seam, 1)
    assert tables.pending is None and tables.last_buf == 1


def test_schedule_rows_are_served_from_its_table(rig):
    tables, seam, built = rig
    cls = torch.tensor([3, 7])
    n = 6
    table = torch.linspace(80.0, 0.1, n)[:, None].expand(n, B).contiguous()
    assert tables.hint_schedule(table, None, cls, None) is True
    (sch,), chain, done = tables.schedules, built[-1], seam.events[-1]
    assert chain.rows == n * B and tables.chains == {n: chain} and sch.done is done
    assert sch.tables.shape == (n, B, WIDTH) and sch.tables.dtype == torch.float32
    assert seam.take() == [("fill", chain, seam.main, n), ("run", chain, sch.tables.data_ptr(), seam.main), ("record", done, seam.main)]
    assert sch.keep[0] is table and sch.others.tensors[1] is cls
    done.complete = True
    # a pending per-step hint and last_buf survive calls served from the schedule
    call(tables, torch.full([B], 9.0), cls)                                 # table 0
    foreign = torch.full([B], 8.0)
    tables.hint_next(foreign, None, cls, None)
    pending, hint_done = tables.pending, seam.events[-1]
    seam.take()
    for i in range(n):
        assert call(tables, table[i], cls) == sch.tables[i].data_ptr()
        assert seam.take() == []                                            # no main_entry, no chain (the event is complete: no wait)
        assert tables.pending is pending and tables.last_buf == 0
        tables.hint_next(table[i], None, cls, None)                         # covered: nothing to do
        assert seam.take() == []
    assert call(tables, foreign, cls) == tables.scales[1].data_ptr()        # the hint is still good
    assert seam.take() == [("wait", seam.main, hint_done), ("record", tables.main_entry, seam.main)]
    # anything that is not a row of the hinted table with the hinted tensors takes the per-step chain
    assert call(tables, table[2].clone(), cls) == tables.scales[0].data_ptr()
    assert seam.take() == inline(tables, seam, 0)
    assert call(tables, table[3], torch.tensor([3, 8])) == tables.scales[1].data_ptr()
    assert seam.take() == inline(tables, seam, 1)
    table[4] *= 0.5                                                         # in place: every row of the record is stale
    assert call(tables, table[1], cls) == tables.scales[0].data_ptr()
    assert seam.take() == inline(tables, seam, 0)
    tables.hint_next(table[1], None, cls, None)                             # ... and no longer covered
    assert [t[0] for t in seam.take()] == ["wait", "fill", "run", "record"]


def test_schedule_tables_are_waited_for_until_seen_complete(rig):
    tables, seam, _ = rig
    cls = torch.tensor([3, 7])
    table = torch.linspace(80.0, 0.1, 6)[:, None].expand(6, B).contiguous()
    tables.hint_schedule(table, None, cls, None)
    (sch,), done = tables.schedules, seam.events[-1]
    seam.take()
    a, b = Stream(seam.trace, "a"), Stream(seam.trace, "b")
    for i, s in enumerate((a, b, a)):                                       # not complete: every call waits, whichever stream it is on
        seam.cur = s
        assert call(tables, table[i], cls) == sch.tables[i].data_ptr()
        assert seam.take() == [("wait", s, done)] and done.queries == i + 1 and not sch.complete
    seam.is_capturing = True                                                # an event cannot be queried under capture: wait
    assert call(tables, table[3], cls) == sch.tables[3].data_ptr()
    assert seam.take() == [("wait", a, done)] and done.queries == 3
    done.complete = True
    assert call(tables, table[3], cls) == sch.tables[3].data_ptr()          # (still capturing: complete or not is unknown)
    assert seam.take() == [("wait", a, done)] and done.queries == 3 and not sch.complete
    seam.is_capturing = False
    seam.cur = b
    assert call(tables, table[4], cls) == sch.tables[4].data_ptr()          # one query sees it complete: no wait
    assert seam.take() == [] and done.queries == 4 and sch.complete
    for s in (a, b, Stream(seam.trace, "c")):                               # from now on neither a query nor a wait, on any stream
        seam.cur = s
        assert call(tables, table[5], cls) == sch.tables[5].data_ptr()
        assert seam.take() == [] and done.queries == 4
    seam.is_capturing = True
    assert call(tables, table[0], cls) == sch.tables[0].data_ptr()          # known complete: capture has nothing to wait for either
    assert seam.take() == [] and done.queries == 4


def test_schedules_and_chains_are_bounded(rig, ct, monkeypatch):
    tables, seam, built = rig
    cls = torch.tensor([3, 7])

    def table(n):
        return torch.linspace(80.0, 0.1, n)[:, None].expand(n, B).contiguous()
    hinted = [table(6) for _ in range(5)]
    for k, t in enumerate(hinted):
        earlier = list(tables.schedules)
        assert len(earlier) == min(k, 4) and tables.hint_schedule(t, None, cls, None)
        chain, done = built[1], seam.events[-1]
        # the chain of the length is reused, behind every kept schedule's event (they share its work buffers)
        assert seam.take() == [("wait", seam.main, sc.done) for sc in earlier] + [
            ("fill", chain, seam.main, 6), ("run", chain, tables.schedules[-1].tables.data_ptr(), seam.main), ("record", done, seam.main)]
    assert len(built) == 2 and ct.SCHEDULES_KEPT == 4
    assert [sc.keep[0] for sc in tables.schedules] == hinted[1:]            # the fifth dropped the first
    # all tables together stay below the bound of a single one: records go from the front
    one = 6 * B * WIDTH * 4
    monkeypatch.setattr(ct, "SCHEDULE_TABLE_MAX_BYTES", 2 * one + one // 2)
    more = table(6)
    assert tables.hint_schedule(more, None, cls, None)
    assert [sc.keep[0] for sc in tables.schedules] == [hinted[4], more]
    # a table over the bound is refused, and nothing happens
    seam.take()
    before = list(tables.schedules)
    assert tables.hint_schedule(table(16), None, cls, None) is False
    assert seam.take() == [] and tables.schedules == before and list(tables.chains) == [6] and len(built) == 2
    # chains by length: the least recently used one goes with the third length
    assert ct.SCHEDULE_CHAINS_KEPT == 2
    tables.hint_schedule(table(3), None, cls, None)
    assert list(tables.chains) == [6, 3] and built[-1].rows == 3 * B
    tables.hint_schedule(table(6), None, cls, None)
    assert list(tables.chains) == [3, 6] and len(built) == 3                # (reused, and the most recent now)
    tables.hint_schedule(table(4), None, cls, None)
    assert list(tables.chains) == [6, 4] and tables.chains[6] is built[1] and tables.chains[4] is built[3]
    assert tables.schedules
    tables.release()
    assert tables.schedules == [] and tables.chains == {}
    seam.take()
    assert call(tables, more[0], cls) == tables.scales[0].data_ptr()        # released: the per-step chain answers
    assert seam.take() == inline(tables, seam, 0)
