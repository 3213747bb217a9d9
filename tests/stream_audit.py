"""TEST INFRASTRUCTURE: happens-before analysis of a recorded multi-stream launch schedule.  Pure Python, no device.

A trace is a list of events in HOST ISSUE ORDER (Trace.launch / record / wait / fork / host_sync).  analyse() gives every stream a
vector clock and proves that every pair of conflicting accesses on different streams is ordered; what it cannot prove is a Conflict.

Stream model (the HIP rules the engine's event rings rely on):
  - launches on one stream run in issue order; a launch ticks its stream's clock;
  - record(e, s) stores s's clock in e, replacing what e held; wait(e, s) joins the snapshot e holds WHEN THE WAIT IS ENQUEUED into
    s's clock -- a later re-record does not move an earlier wait; a wait on a never-recorded event is a no-op;
  - fork(a, b) = record + wait on a private event;
  - host_sync(s) makes everything queued on s so far precede every later event of every stream (ALL: of all streams;
    EventRef(e): everything e holds, the host-side wait for an event);
  - no stream is ordered with another implicitly: the default stream is a stream like any other (non-blocking streams).

Regions are byte ranges ("range", lo, hi) or rectangles ("rect", base, rows, row_bytes, pitch_bytes).  Two rectangles of equal pitch
overlap exactly (row r of one against row r' of the other); any other pair overlaps when the bounding ranges do.

Access modes: r, w, rw, acc (a commutative atomic accumulation).  acc with acc never conflicts; acc against anything else counts as rw.
A read must follow the last write of what it reads; a write must follow the last write and every read since.  An address is an
address: memory handed from one tensor to the next by an allocator is not special.
"""
from collections import namedtuple

ALL = "ALL"
MODES = ("r", "w", "rw", "acc")

Launch = namedtuple("Launch", "stream accesses name site")          # accesses: [(region, mode, argument name)]
Record = namedtuple("Record", "event stream site")
Wait = namedtuple("Wait", "event stream site")
Fork = namedtuple("Fork", "src dst site")
HostSync = namedtuple("HostSync", "stream site")
EventRef = namedtuple("EventRef", "event")                          # host_sync(EventRef(e)): the host waits for what e holds (hipEventSynchronize)
Mark = namedtuple("Mark", "label")                                  # a label in the trace (step boundaries); orders nothing

Edge = namedtuple("Edge", "index kind src dst site")                # an ordering event of the trace: kind wait / fork / host_sync
Conflict = namedtuple("Conflict", "kind first second")              # kind: RAW / WAR / WAW; first / second: Access in issue order


class Access:
    """one argument of one launch: index = position of the launch in the trace, tick = its stream's clock value"""
    __slots__ = ("index", "stream", "tick", "name", "arg", "mode", "region", "site", "dead")

    def __init__(self, index, stream, tick, name, arg, mode, region, site):
        self.index, self.stream, self.tick, self.name, self.arg, self.mode, self.region, self.site = \
            index, stream, tick, name, arg, mode, region, site
        self.dead = False


def rng(lo, hi):
    return ("range", int(lo), int(hi))


def rect(base, rows, row_bytes, pitch_bytes):
    """rows x row_bytes bytes, row r at base + r * pitch_bytes; a gapless or single-row rectangle is the byte range it covers"""
    base, rows, row_bytes, pitch_bytes = int(base), int(rows), int(row_bytes), int(pitch_bytes)
    if rows <= 0 or row_bytes <= 0:
        return ("range", base, base)
    if rows == 1 or row_bytes >= pitch_bytes:
        return ("range", base, base + (rows - 1) * pitch_bytes + row_bytes)
    return ("rect", base, rows, row_bytes, pitch_bytes)


def bounds(region):
    if region[0] == "range":
        return region[1], region[2]
    _, base, rows, rb, pitch = region
    return base, base + (rows - 1) * pitch + rb


def overlap(a, b):
    alo, ahi = bounds(a)
    blo, bhi = bounds(b)
    if alo >= bhi or blo >= ahi:
        return False
    if a[0] == "rect" and b[0] == "rect" and a[4] == b[4]:
        # row i of b starts d + i * pitch bytes behind row 0 of a; row j of a covers [j * pitch, j * pitch + wa): rows i, j meet when
        # -wb < d + (i - j) * pitch < wa for some k = i - j in [-(rows_a - 1), rows_b - 1]
        pitch, d, wa, wb = a[4], b[1] - a[1], a[3], b[3]
        kmin = (-wb - d) // pitch + 1
        kmax = -((d - wa) // pitch) - 1
        return max(kmin, -(a[2] - 1)) <= min(kmax, b[2] - 1)
    return True


def covers(a, b):
    """every byte of b is a byte of a (sufficient condition)"""
    blo, bhi = bounds(b)
    if a[0] == "range":
        return a[1] <= blo and bhi <= a[2]
    if b[0] == "rect" and a[4] == b[4]:
        d = b[1] - a[1]
        r0, c0 = divmod(d, a[4])
        return d >= 0 and c0 + b[3] <= a[3] and r0 + b[2] <= a[2]
    return False


class Trace:
    def __init__(self):
        self.events = []

    def launch(self, stream, accesses, name="", site=""):
        acc = []
        for a in accesses:
            region, mode = a[0], a[1]
            assert mode in MODES, mode
            acc.append((region, mode, a[2] if len(a) > 2 else ""))
        self.events.append(Launch(stream, acc, name, site))

    def record(self, event, stream, site=""):
        self.events.append(Record(event, stream, site))

    def wait(self, event, stream, site=""):
        self.events.append(Wait(event, stream, site))

    def fork(self, src, dst, site=""):
        self.events.append(Fork(src, dst, site))

    def host_sync(self, stream=ALL, site=""):
        self.events.append(HostSync(stream, site))

    def mark(self, label):
        self.events.append(Mark(label))

    def extend(self, events):
        self.events.extend(events)


def edges(trace):
    """the ordering events of a trace: every wait (src = the stream of the record it binds to; a wait that binds to nothing is no
    edge), fork and host_sync (dst = ALL)"""
    out, last = [], {}
    for i, ev in enumerate(trace.events):
        if isinstance(ev, Record):
            last[ev.event] = ev.stream
        elif isinstance(ev, Wait):
            if ev.event in last and last[ev.event] != ev.stream:
                out.append(Edge(i, "wait", last[ev.event], ev.stream, ev.site))
        elif isinstance(ev, Fork):
            if ev.src != ev.dst:
                out.append(Edge(i, "fork", ev.src, ev.dst, ev.site))
        elif isinstance(ev, HostSync):
            out.append(Edge(i, "host_sync", ev.stream, ALL, ev.site))
    return out


def without(trace, removed):
    """the same trace with the ordering events `removed` (Edge objects or event indices) deleted from the model"""
    drop = {e.index if isinstance(e, Edge) else int(e) for e in removed}
    for i in drop:
        assert isinstance(trace.events[i], (Wait, Fork, HostSync)), f"event {i} orders nothing: {trace.events[i]}"
    t = Trace()
    t.events = [ev for i, ev in enumerate(trace.events) if i not in drop]
    return t


def _join(a, b):
    for k, v in b.items():
        if a.get(k, 0) < v:
            a[k] = v


class Report:
    def __init__(self):
        self.conflicts = []          # distinct (kind, both names / arguments / sites / streams): the first instance of each
        self.counts = {}             # the same key -> number of instances
        self.launches = 0
        self.streams = set()
        self.n_edges = 0
        self.pairs_checked = 0       # overlapping accesses on different streams, at least one of them a write, that had to be ordered

    @property
    def ok(self):
        return not self.conflicts

    def describe(self, limit=20):
        lines = [f"{len(self.conflicts)} distinct conflicts ({sum(self.counts.values())} instances), {self.launches} launches, "
                 f"{len(self.streams)} streams, {self.n_edges} ordering edges, {self.pairs_checked} cross-stream pairs checked"]
        for c in self.conflicts[:limit]:
            a, b = c.first, c.second
            lines.append(f"  {c.kind}: {a.name}({a.arg}:{a.mode}) on stream {a.stream:#x} at {a.site}  !<  "
                         f"{b.name}({b.arg}:{b.mode}) on stream {b.stream:#x} at {b.site}   x{self.counts[_ckey(c)]}")
        return "\n".join(lines)


def _ckey(c):
    a, b = c.first, c.second
    return (c.kind, a.name, a.arg, a.site, a.stream, b.name, b.arg, b.site, b.stream)


PAGE = 16                                # log2 of the address bucket of the access index


def analyse(trace):
    """-> Report.  Every access is checked against the earlier accesses it overlaps that are still LIVE: an access is retired once a
    later access that happens after it covers it and demands at least as much order of its successors (a write retires anything; a
    read retires reads, an accumulation accumulations) -- whatever must follow the retired one must follow its successor anyway."""
    rep = Report()
    clock, held, host = {}, {}, {}
    pages = {}                           # address bucket -> live accesses (an access sits in every bucket its bounding range meets)
    n_fork = 0

    def touch(s):
        c = clock.setdefault(s, {})
        _join(c, host)
        rep.streams.add(s)
        return c

    def do_record(e, s):
        held[e] = dict(touch(s))

    def do_wait(e, s):
        c = touch(s)
        if e in held:
            _join(c, held[e])

    for index, ev in enumerate(trace.events):
        if isinstance(ev, Launch):
            c = touch(ev.stream)
            c[ev.stream] = tick = c.get(ev.stream, 0) + 1
            rep.launches += 1
            new = []
            for region, mode, arg in ev.accesses:
                lo, hi = bounds(region)
                if hi <= lo:
                    continue
                me = Access(index, ev.stream, tick, ev.name, arg, mode, region, ev.site)
                seen = set()
                for p in range(lo >> PAGE, ((hi - 1) >> PAGE) + 1):
                    live = pages.get(p)
                    if not live:
                        continue
                    for old in live:
                        if old.dead or id(old) in seen:
                            continue
                        seen.add(id(old))
                        if old.index == index or not overlap(old.region, region):
                            continue
                        before = old.stream == ev.stream or c.get(old.stream, 0) >= old.tick
                        need = not (old.mode == "r" and mode == "r") and not (old.mode == "acc" and mode == "acc")
                        if need and old.stream != ev.stream:
                            rep.pairs_checked += 1
                            if not before:
                                kind = "RAW" if mode == "r" else "WAR" if old.mode == "r" else "WAW"
                                cf = Conflict(kind, old, me)
                                k = _ckey(cf)
                                if k not in rep.counts:
                                    rep.conflicts.append(cf)
                                rep.counts[k] = rep.counts.get(k, 0) + 1
                        if before and covers(region, old.region) and (mode in ("w", "rw") or mode == old.mode):
                            old.dead = True
                    if any(o.dead for o in live):
                        pages[p] = [o for o in live if not o.dead]
                new.append(me)
            for me in new:
                lo, hi = bounds(me.region)
                for p in range(lo >> PAGE, ((hi - 1) >> PAGE) + 1):
                    pages.setdefault(p, []).append(me)
        elif isinstance(ev, Record):
            do_record(ev.event, ev.stream)
        elif isinstance(ev, Wait):
            do_wait(ev.event, ev.stream)
        elif isinstance(ev, Fork):
            n_fork += 1
            do_record(("fork", n_fork), ev.src)
            do_wait(("fork", n_fork), ev.dst)
        elif isinstance(ev, HostSync):
            if ev.stream == ALL:
                for s in list(clock):
                    _join(host, touch(s))
            elif isinstance(ev.stream, EventRef):
                _join(host, held.get(ev.stream.event, {}))
            else:
                _join(host, touch(ev.stream))
    rep.n_edges = len(edges(trace))
    return rep
