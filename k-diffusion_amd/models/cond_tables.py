"""Where a forward's AdaRMSNorm scale table comes from, and the only place of the package that orders work across HIP streams.

A launch plan keeps one ``ScaleTables`` (``plan.tables``).  The [B, scale_width] table of a model call is, in this order of preference,

* a row of a whole-schedule table (``hint_schedule``: one conditioning chain over all steps x B rows, ahead of the solver loop);
* the ping-pong table a side stream filled one step ahead (``hint_next``);
* the per-step chain, run inline on the caller's stream.

All three run the same row-by-row kernels, so the scales are the same bits whichever answers.  The object sees streams and events only
through a small seam (``TorchStreams`` by default) and conditioning chains only as ``fill(...)`` / ``run(table_ptr, stream)``, so the whole
state machine runs on the CPU under recording fakes (tests/test_cond_tables_cpu.py).
"""
import ctypes as C

import torch

from .. import weights

# Largest [steps, B, scale_width] scale table kept per sigma schedule (hint_schedule); longer schedules use the per-step chain.
SCHEDULE_TABLE_MAX_BYTES = 1 << 30
SCHEDULES_KEPT = 4            # a run of a two-stage solver hints two tables; older records (and their tensors) are dropped
SCHEDULE_CHAINS_KEPT = 2      # conditioning workspaces kept per plan, by schedule length (least recently used dropped)


class TorchStreams:
    """The stream seam on torch's HIP streams.  Streams answer ``wait_event(event)``, events ``record(stream)`` and ``query()``."""

    current = staticmethod(torch.cuda.current_stream)
    side = staticmethod(torch.cuda.Stream)                          # side(device=...): a new stream
    event = staticmethod(torch.cuda.Event)
    on = staticmethod(torch.cuda.stream)                            # with on(s): s is the current stream inside
    capturing = staticmethod(torch.cuda.is_current_stream_capturing)

    @staticmethod
    def handle(stream):
        return C.c_void_p(stream.cuda_stream)


def idents(*tensors):
    return tuple(map(weights.ident, tensors))


class _Held:
    """The conditioning tensors a table was computed from.  The record keeps them alive: while it exists their storage cannot be freed
    and handed to another tensor, so a later call whose (address, version, shape) keys match really passes the same data."""

    def __init__(self, *tensors):
        self.tensors, self.idents = tensors, idents(*tensors)

    def same(self, idents):
        return self.idents == idents


class _Schedule:
    """Scale tables of a whole sigma schedule: rows of ``sigma_table`` ([n, B], one row per model call) -> tables[i]."""

    def __init__(self, sigma_table, others, tables, done):
        self.base, self.version, (self.n, self.B) = weights.ident(sigma_table)
        self.others, self.tables, self.done = others, tables, done      # others: _Held (aug_cond, class_cond, mapping_cond)
        self.complete = False     # ``done`` was seen complete once: the tables are in memory for every stream, nobody waits again
        self.keep = (sigma_table, others)

    def row_of(self, sigma):
        """Index of the table row ``sigma`` is a view of, or None."""
        if sigma.dtype != torch.float32 or sigma.numel() != self.B or not sigma.is_contiguous() or weights.version(sigma) != self.version:
            return None
        off = sigma.data_ptr() - self.base
        if off < 0 or off % (4 * self.B) or off // (4 * self.B) >= self.n:
            return None
        return off // (4 * self.B)


class ScaleTables:
    """The scale tables of one plan: two ping-pong [B, scale_width] tables with the per-step chain, the side stream that fills one of
    them a step ahead, and the tables (and chains, by length) of hinted sigma schedules.  ``build_chain(rows)`` makes a conditioning
    chain with its own input and work buffers."""

    def __init__(self, B, scale_width, device, build_chain, streams=TorchStreams):
        self.B, self.scale_width, self.build_chain, self.streams = B, scale_width, build_chain, streams
        # ping-pong: the main chain reads one table while the next step's is being written
        self.scales = [torch.empty(B, scale_width, device=device, dtype=torch.float32) for _ in range(2)]
        self.last_buf, self.pending = 1, None               # pending: (_Held conditioning tensors, table, done event) of an unused hint
        self.side_stream = streams.side(device=device)
        self.main_entry = streams.event()
        self.entered = None                                 # stream of a call whose table is no schedule's, until ``mark_entry``
        self.schedules, self.chains = [], {}                # whole sigma schedules (hint_schedule); their chains by length
        self.step_chain = build_chain(B)                    # the per-step chain (inline, or one step ahead on the side stream)

    def _covering(self, sigma, others):
        """(schedule, row) of the first schedule that holds ``sigma`` as a row and was hinted with the tensors ``others`` names."""
        for sch in self.schedules:
            i = sch.row_of(sigma) if sch.others.same(others) else None
            if i is not None:
                return sch, i
        return None, None

    def table_for(self, sigma, aug_cond, class_cond, mapping_cond):
        """Address of this call's [B, scale_width] table; whatever fills it is ordered in front of the current stream's later work."""
        st = self.streams
        ident = idents(sigma, aug_cond, class_cond, mapping_cond)
        sch, i = self._covering(sigma, ident[1:])
        if sch is not None:                       # this call's scales were computed with its whole sigma schedule
            # the table was computed once, ahead of the loop, on the stream that was current in hint_schedule.  Forwards wait for it
            # until one of them sees the event complete; from then on the table is in memory for every stream (a wait packet per
            # forward costs ~3 us of idle queue each: profiles/r06_launch_gaps_*.txt).  An event cannot be queried under capture.
            if not sch.complete:
                if not st.capturing() and sch.done.query():
                    sch.complete = True
                else:
                    st.current().wait_event(sch.done)
            self.entered = None                   # (a pending per-step hint and last_buf stay as they are)
            return sch.tables[i].data_ptr()
        cur = st.current()
        pre, self.pending = self.pending, None
        if pre is not None and pre[0].same(ident):
            buf = pre[1]                          # this step's scale table was computed ahead of time on the side stream
            cur.wait_event(pre[2])
        else:
            buf = 1 - self.last_buf
            if pre is not None:
                cur.wait_event(pre[2])            # an unused hint still owns the conditioning workspace: order behind it
            self.step_chain.fill(sigma, aug_cond, class_cond, mapping_cond)
            self.step_chain.run(self.scales[buf].data_ptr(), st.handle(cur))
        self.last_buf, self.entered = buf, cur
        return self.scales[buf].data_ptr()

    def mark_entry(self):
        """The caller has enqueued everything that precedes its main chain: the side stream's next chain may start behind this point.
        (Only that chain waits on the event, so a call served from a schedule records nothing.)"""
        if self.entered is not None:
            self.main_entry.record(self.entered)
            self.entered = None

    def hint_next(self, sigma, aug_cond, class_cond, mapping_cond):
        """The NEXT call will pass exactly these tensors: unless a hint is pending or a schedule covers that call, its chain runs on
        the side stream, beside the main chain of the step in flight, into the other table."""
        if self.pending is not None or self._covering(sigma, idents(aug_cond, class_cond, mapping_cond))[0] is not None:
            return
        st = self.streams
        buf = 1 - self.last_buf
        side = self.side_stream
        side.wait_event(self.main_entry)          # table `buf` and the conditioning workspace are free once the main chain of
        with st.on(side):                         # the step in flight has started (its predecessors are complete in stream order)
            self.step_chain.fill(sigma, aug_cond, class_cond, mapping_cond)
            self.step_chain.run(self.scales[buf].data_ptr(), st.handle(side))
            done = st.event()
            done.record(side)
        # (a sampler aborted mid-loop leaves the record behind; the next run's schedule then necessarily lives at other addresses)
        self.pending = (_Held(sigma, aug_cond, class_cond, mapping_cond), buf, done)

    def hint_schedule(self, sigma_table, aug_cond, class_cond, mapping_cond):
        """Calls of this run will pass rows of ``sigma_table`` ([n, B] fp32, contiguous) with exactly these other tensors: one chain
        over all n x B rows on the current stream, now.  False when the table would exceed SCHEDULE_TABLE_MAX_BYTES."""
        n, B = sigma_table.shape
        if n * B * self.scale_width * 4 > SCHEDULE_TABLE_MAX_BYTES:
            return False
        chain = self.chains.pop(n, None)
        if chain is None:
            with torch.inference_mode(False):
                chain = self.build_chain(n * B)
        self.chains[n] = chain                    # most recently used last; older lengths (and their workspaces) are dropped
        for old_n in list(self.chains)[:-SCHEDULE_CHAINS_KEPT]:
            del self.chains[old_n]
        st = self.streams
        cur = st.current()
        for sch in self.schedules:                # an earlier schedule's chain of the same length shares the work buffers
            cur.wait_event(sch.done)
        tables = torch.empty(n, B, self.scale_width, device=sigma_table.device, dtype=torch.float32)
        chain.fill(sigma_table, aug_cond, class_cond, mapping_cond, repeat=n)
        chain.run(tables.data_ptr(), st.handle(cur))
        done = st.event()
        done.record(cur)
        self.schedules.append(_Schedule(sigma_table, _Held(aug_cond, class_cond, mapping_cond), tables, done))
        del self.schedules[:-SCHEDULES_KEPT]
        while len(self.schedules) > 1 and sum(sc.tables.numel() * 4 for sc in self.schedules) > SCHEDULE_TABLE_MAX_BYTES:
            del self.schedules[0]                 # all tables of a plan together stay below the bound of a single one
        return True

    def release(self):
        """Drop the schedules' tables (with the hinted tensors they keep alive) and chains."""
        self.schedules.clear()
        self.chains.clear()
