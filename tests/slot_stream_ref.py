"""The reference of the slots streams (TEST INFRASTRUCTURE, a plain helper module beside tests/stream_ref.py and
tests/mfn_stream_ref.py): sequences that are seated in, and released from, the slots of one batch at different calls.

It adds no arithmetic of its own.  A SCHEDULE is a list of events ``(call, slot, "seat" | "release", recording)``: before call ``call``
the slot is seated with recording number ``recording`` (its window 0 is the next one) or released (``recording`` is None).
``timetable`` turns it into, per call and slot, the (recording, window) that the call computes, or None where the slot is idle or
full; every seated recording is then run ALONE, as a batch of one, through the existing references (``stream_ref.encoder_stack``,
``mfn_stream_ref.mfn_gate``), and its rows are put where the timetable says.  Idle and full calls give zero rows.  With
``rounding=False`` underneath it is the exact function (tests/test_slot_stream_cpu.py).
"""
import torch

import mfn_stream_ref as M
import stream_ref as S


def timetable(schedule, n_calls, n_slots, limit=None):
    """-> table[call][slot] = (recording, window) or None; positions[call][slot] = the slot's position BEFORE the call, as the device
    holds it: -1 idle, the next window otherwise (``limit`` once the recording has used the whole capacity: such a slot is full, its
    rows are zeros and it stays where it is)."""
    table, positions = [], []
    cur = [None] * n_slots                                   # [recording, next window]
    for call in range(n_calls):
        for c, slot, what, rec in schedule:
            if c != call:
                continue
            assert what in ("seat", "release") and 0 <= slot < n_slots, (c, slot, what)
            cur[slot] = [rec, 0] if what == "seat" else None
        row = []
        positions.append([-1 if s is None else s[1] for s in cur])
        for s in cur:
            if s is None or (limit is not None and s[1] >= limit):
                row.append(None)
            else:
                row.append((s[0], s[1]))
                s[1] += 1
        table.append(row)
    return table, positions


def windows_used(table):
    """{recording: how many of its windows the timetable computes}"""
    used = {}
    for row in table:
        for cell in row:
            if cell is not None:
                used[cell[0]] = max(used.get(cell[0], 0), cell[1] + 1)
    return used


def assemble(table, alone, width, dtype=torch.float64):
    """alone {recording: (windows, width)} -> (calls, slots, width): each computed cell from its recording's own rows, zeros elsewhere"""
    out = torch.zeros(len(table), len(table[0]), width, dtype=dtype)
    for call, row in enumerate(table):
        for slot, cell in enumerate(row):
            if cell is not None:
                out[call, slot] = alone[cell[0]][cell[1]]
    return out


def call_inputs(table, recordings, idle):
    """What the caller feeds call by call: recordings {recording: (T, width)} -> (calls, slots, width), a computed cell getting its
    recording's window and every other cell the row ``idle`` (width) (any values: such a cell must not reach a result)."""
    rec0 = next(iter(recordings.values()))
    out = idle.to(rec0.dtype).reshape(1, 1, -1).repeat(len(table), len(table[0]), 1)
    for call, row in enumerate(table):
        for slot, cell in enumerate(row):
            if cell is not None:
                out[call, slot] = recordings[cell[0]][cell[1]]
    return out


def encoder_slots(p, prefix, h, x, mask, table, rounding=True):
    """x {recording: (T, d)}, mask {recording: (T,)} or None -> (calls, slots, d): every recording alone through stream_ref"""
    alone = {}
    for rec, n in windows_used(table).items():
        m = None if mask is None else mask[rec][:n].reshape(1, n, 1)
        alone[rec] = S.encoder_stack(p, prefix, x[rec][:n].unsqueeze(0), m, h, rounding)[0]
    d = next(iter(x.values())).shape[-1]
    return assemble(table, alone, d)


def mfn_slots(p, prefix, mods, x, mask, table, rounding=True, output_dim=1):
    """x {recording: {mod: (T, d_mod)}}, mask {recording: (T,)} or None -> (calls, slots, output_dim): every recording alone through
    mfn_stream_ref (the mask multiplies the output row; the state advances under a blanked window)"""
    alone = {}
    for rec, n in windows_used(table).items():
        m = None if mask is None else mask[rec][:n].reshape(1, n, 1)
        alone[rec] = M.mfn_gate(p, prefix, {k: x[rec][k][:n].unsqueeze(1) for k in mods}, mods, m, rounding)[0]
    return assemble(table, alone, output_dim)
