"""The rules of DESIGN.md 4.21 for the entropy data of a JPEG file without restart markers cut into pieces, in plain Python: a second
statement of what csrc/jpeg_sync.hpp computes, written from the rules and not from that code. `info(data, piece_bytes)` -> (mode,
pieces, groups), what dad3d_jpeg_decode_sync and dad3d_jpeg_decode_sync_host report for the file: (0, 0, 0) for a file the header
walk or the segment table flags and for a file with a restart interval; else mode 1 for a file whose hand-over is verified, 2 for any
other.

A position here counts data bits (the stuffed 00 bytes taken out), which is the rule "no position rests on a stuffed byte" made a
coordinate: it rises with the position in the file, so "the code's first bit lies in the piece's bytes" and "two states are equal"
mean the same in both. A group's rounds have one fixed point, the chain of its pieces from the group's input, and a chain of pieces
is one walk that stops at the first state at or behind the group's last byte; so a group is one walk here."""
import bisect

import jpeg_restatement as R

GROUP = 256
END = "END"


class Scan:
    """The entropy bytes [scan_at, scan_end) of a file: its data bits, and where each data byte lay."""

    def __init__(self, raw):
        self.size = len(raw)
        self.raw_of = [i for i in range(len(raw)) if not (i > 0 and raw[i] == 0 and raw[i - 1] == 0xFF)]
        self.bits = "".join(format(raw[i], "08b") for i in self.raw_of)

    def first_bit(self, byte):
        """The first data bit at or behind the byte: where a piece that starts there begins, and where the piece in front ends."""
        return 8 * bisect.bisect_left(self.raw_of, byte)


def walk(scan, tables, state, stop):
    """The lenient walk from `state` = (bit, j, k) over the codes that begin in front of the data bit `stop`; the state it hands on."""
    if state == END:
        return END
    bits, total = scan.bits, len(scan.bits)
    t, j, k = state
    while t < stop:
        codes, lengths = tables[j]["dc" if k == 0 else "ac"]
        peek = bits[t:t + 16].ljust(16, "0")
        found = next(((codes[peek[:n]], n) for n in lengths if peek[:n] in codes), None)
        if found is None:  # a code no table assigns costs one bit
            if t + 1 > total:
                return END
            t += 1
            continue
        symbol, used = found
        size = symbol if k == 0 else symbol & 15
        if t + used > total or t + used + size > total:
            return END
        t += used + size
        if k == 0:
            k = 1
        elif size == 0:
            k = k + 16 if symbol >> 4 == 15 else 64
        else:
            k += (symbol >> 4) + 1
        if k >= 64:
            j, k = (j + 1) % len(tables), 0
    return (t, j, k)


def layout(data):
    """(Scan, the tables by block of the MCU) of a file without restart markers, or None."""
    try:
        hd = R.parse(data)
        h, w, comps = hd["sof"]
        if hd["interval"]:
            return None
        mcus = -(-w // (8 * comps[0]["h"])) * -(-h // (8 * comps[0]["v"]))
        (start, end), = R.segments(data, hd, mcus)
    except R.Flag:
        return None
    return Scan(data[start:end]), [comp for comp in comps for _ in range(comp["h"] * comp["v"])]


def exits(data, piece_bytes):
    """(pieces, [exit of every group behind launch A], [behind launch B]) or None."""
    found = layout(bytes(data))
    if found is None:
        return None
    scan, tables = found
    pieces = max(1, -(-scan.size // piece_bytes))
    groups = -(-pieces // GROUP)
    span = GROUP * piece_bytes
    stops = [scan.first_bit(min((g + 1) * span, scan.size)) for g in range(groups)]
    guess = [(scan.first_bit(g * span), 0, 0) for g in range(groups)]
    exit_a = [walk(scan, tables, guess[g], stops[g]) for g in range(groups)]
    exit_b = [walk(scan, tables, exit_a[g - 1] if g else guess[0], stops[g]) for g in range(groups)]
    return pieces, exit_a, exit_b


def info(data, piece_bytes):
    found = exits(data, piece_bytes)
    if found is None:
        return (0, 0, 0)
    pieces, exit_a, exit_b = found
    return (1 if exit_a == exit_b else 2, pieces, len(exit_a))
