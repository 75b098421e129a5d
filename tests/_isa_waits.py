"""Helper of tests/test_isa_nb_pipeline.py: disassembles the gfx950 code object of the built library and walks a kernel's chunk loop
with a model of the vector-memory counter.

The model: on gfx950 `vmcnt` counts global loads AND stores and retires them in order, so the outstanding operations form a queue;
`global_load*` / `global_store*` push one entry, `s_waitcnt vmcnt(N)` retires the oldest entries until N remain.  A walk follows the
hot path of a loop: conditional branches fall through (the compiler lays the unlikely blocks out of line), except a conditional branch
to the loop header, which is the back edge; unconditional branches are followed."""
import os
import re
import shutil
import subprocess

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


class Ins:
    __slots__ = ("addr", "text", "op", "target")

    def __init__(self, addr, text):
        self.addr, self.text = addr, text
        self.op = text.split()[0]
        self.target = None
        if self.op == "s_branch" or self.op.startswith("s_cbranch"):
            off = int(text.split()[1])
            off = off - 65536 if off >= 32768 else off   # simm16, in dwords from the next instruction
            self.target = addr + 4 + 4 * off

    def __repr__(self):
        return f"{self.addr:x}: {self.text}"


def disassemble(lib_path, workdir):
    """{kernel symbol: [Ins, ...]} of the gfx950 code object inside the library"""
    so = shutil.copy(lib_path, os.path.join(workdir, "lib.so"))
    subprocess.run([OBJDUMP, "--offloading", str(so)], check=True, capture_output=True, cwd=workdir)
    co = [f for f in os.listdir(workdir) if "gfx950" in f]
    assert co, "no gfx950 code object inside the library"
    out = subprocess.run([OBJDUMP, "-d", os.path.join(workdir, co[0])], check=True, capture_output=True, text=True).stdout
    funcs, name = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            funcs[name] = []
        elif name is not None and line.startswith("\t"):
            text, _, comment = line.strip().partition("//")
            a = re.match(r"\s*([0-9A-Fa-f]+):", comment)
            if text.strip() and a:
                funcs[name].append(Ins(int(a.group(1), 16), text.strip()))
    return funcs


def vmcnt_of(text):
    """the vmcnt field of an s_waitcnt, None if it has none"""
    m = re.search(r"vmcnt\((\d+)\)", text)
    return int(m.group(1)) if (text.startswith("s_waitcnt") and m) else None


def _regs(operand):
    """the VGPR numbers an operand such as v7 or v[4:5] names"""
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def find_chunk_loop(ins):
    """(header index, back-edge index) of the innermost loop that holds both MFMAs and global stores: the smallest backward-branch
    span [target, branch] with at least one v_mfma and one global_store inside"""
    at = {x.addr: i for i, x in enumerate(ins)}
    best = None
    for i, x in enumerate(ins):
        if x.target is not None and x.target <= x.addr and x.target in at:
            h = at[x.target]
            body = ins[h:i + 1]
            if any(b.op.startswith("v_mfma") for b in body) and any(b.op.startswith("global_store") for b in body):
                if best is None or i - h < best[1] - best[0]:
                    best = (h, i)
    assert best is not None, "no loop with MFMAs and global stores"
    return best


def hot_trip(ins, header):
    """indices of the instructions on one hot-path trip of the loop that starts at index `header`, back edge included"""
    at = {x.addr: i for i, x in enumerate(ins)}
    trip, i = [], header
    while True:
        assert len(trip) < 20000, "the walk does not return to the loop header"
        x = ins[i]
        trip.append(i)
        if x.op == "s_branch" or (x.op.startswith("s_cbranch") and x.target == ins[header].addr):
            i = at[x.target]
            if i == header:
                return trip
        else:
            i += 1
            if i == header:
                return trip


def walk(ins, trip, trips=3):
    """Runs the queue model over `trips` consecutive trips (the first only fills the queue) and returns the events of the later, steady
    ones: a list of dicts
       {"kind": "wait", "ins", "chunk", "retired": [entries]}    entry = {"kind": "load" | "store", "chunk", "dst": set of VGPRs}
       {"kind": "mov_of_load", "ins", "chunk", "entry"}          a v_mov whose source is the destination of a queued load
       {"kind": "wait_before_mfma", "ins", "chunk"}              an s_waitcnt with a vmcnt field after a chunk's last store, before the next v_mfma
       {"kind": "mov_of_chunk_load", "ins", "chunk", "load"}     a v_mov from a register that a load issued in the SAME chunk wrote last, waited for
                                                                 or not (compiled code always waits first, so "mov_of_load" cannot fire on it)
    Chunks are numbered along the walk: a chunk ends at the first v_mfma that follows a gradient store."""
    queue, events, after_store = [], [], []
    chunk, stores_seen, fresh = 0, False, {}   # fresh: VGPR -> the load of the current chunk that wrote it last
    for t in range(trips):
        steady = t > 0
        for i in trip:
            x = ins[i]
            if x.op.startswith("v_mfma") and stores_seen:
                events += after_store   # the waits since the chunk's LAST store
                chunk, stores_seen, after_store, fresh = chunk + 1, False, [], {}
            if x.op.startswith("v_mov_b") and steady:
                for r in _regs(x.text.split(None, 1)[1].split(",")[1].strip()):
                    if r in fresh:
                        events.append({"kind": "mov_of_chunk_load", "ins": x, "chunk": chunk, "load": fresh[r]})
            if len(x.text.split()) > 1 and not x.op.startswith("global_store"):   # whatever this instruction writes is no load's value any more
                for r in _regs(x.text.split()[1].rstrip(",")):
                    fresh.pop(r, None)
            if x.op.startswith("global_load"):
                queue.append({"kind": "load", "chunk": chunk, "dst": _regs(x.text.split()[1].rstrip(",")), "ins": x})
                fresh.update({r: x for r in queue[-1]["dst"]})
            elif x.op.startswith("global_store"):
                queue.append({"kind": "store", "chunk": chunk, "dst": set(), "ins": x})
                stores_seen, after_store = True, []
            elif vmcnt_of(x.text) is not None:
                n = vmcnt_of(x.text)
                retired = queue[:max(0, len(queue) - n)]
                del queue[:len(retired)]
                if steady:
                    events.append({"kind": "wait", "ins": x, "chunk": chunk, "retired": retired})
                    if stores_seen:
                        after_store.append({"kind": "wait_before_mfma", "ins": x, "chunk": chunk})
            elif x.op.startswith("v_mov_b") and steady:
                src = set().union(*[_regs(o.strip()) for o in x.text.split(None, 1)[1].split(",")[1:]])
                for e in queue:
                    if e["kind"] == "load" and e["dst"] & src:
                        events.append({"kind": "mov_of_load", "ins": x, "chunk": chunk, "entry": e})
            # any other instruction that overwrites a queued load's destination is not modelled: the compiler waits before it
    return events
