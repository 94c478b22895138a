"""Static check of an hipcc -S listing for the hazards an inline-asm MFMA kernel has to avoid by construction (hipcc does not know that the asm
statements are MFMAs, so it pads none of their wait states).  Only MFMAs inside ;;#ASMSTART ... ;;#ASMEND are tracked: the MFMAs hipcc
schedules itself (builtins) are padded by its own hazard recogniser.  A kernel without any asm markers (a listing they were stripped from)
gives no way to tell the two apart, so there every MFMA is tracked, as before the markers were read.  Rules, for an asm MFMA still in flight (fewer than MIN_GAP MFMA issues,
each >= 32 cycles for 32x32x16, and fewer than SETTLE wait states behind it):
  read   a non-MFMA instruction READS a register the MFMA writes (stale data);
  waw    a non-MFMA instruction WRITES a register the MFMA writes (the MFMA's late write lands on top of it);
  war    a non-MFMA instruction WRITES a register the MFMA reads as C (the MFMA reads the new value);
and a VALU / accvgpr write to a register that an asm MFMA reads as A / B / C directly in front of it (< 2 wait states: late write).
The listing is scanned in order; the state at a branch is carried to the branch's target label, forward (merged with the fall-through)
and backward (the loop head is replayed with the state of the loop's tail until it settles).
Usage: python tools/check_mfma_hazards.py listing.s [kernel-name-substring]"""
import re
import sys

MIN_GAP = 2
SETTLE = 20  # wait states that settle any MFMA
LATE = 3  # a write must be at least LATE - 1 wait states ahead of the MFMA that reads it

_STORE = ("buffer_store", "global_store", "scratch_store", "flat_store", "ds_write")


def regs(tok):
    m = re.fullmatch(r"([va])\[(\d+):(\d+)\]", tok)
    if m:
        return {(m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)}
    m = re.fullmatch(r"([va])(\d+)", tok)
    if m:
        return {(m.group(1), int(m.group(2)))}
    return set()


def parse(line):
    line = line.split(";")[0].strip()
    if not line or line.startswith(".") or line.endswith(":"):
        return None
    parts = line.replace(",", " ").split()
    op, toks = parts[0], parts[1:]
    return op, [regs(t) for t in toks], toks


def kernels(text):
    """{kernel symbol: [(line no, raw line, inside an asm statement)]} for every _Z... label of the listing (the whole listing if it has none).
    In a kernel without any ;;#ASMSTART marker every line counts as inside one."""
    out, cur, name, in_asm, marked = {}, None, None, False, set()
    for ln, raw in enumerate(text.split("\n"), 1):
        m = re.match(r"^(_Z\w+):", raw)
        if m:
            name, cur, in_asm = m.group(1), [], False
            out[name] = cur
            continue
        if raw.startswith(".Lfunc_end"):
            cur = None
            continue
        if "#ASMSTART" in raw:
            in_asm = True
            marked.add("" if name is None else name)
            continue
        if "#ASMEND" in raw:
            in_asm = False
            continue
        if cur is None:
            if name is None:
                cur = out.setdefault("", [])
            else:
                continue
        cur.append((ln, raw, in_asm))
    for k, body in out.items():
        if k not in marked:
            out[k] = [(ln, raw, True) for ln, raw, _ in body]
    return out


class _State:
    """pending: in-flight asm MFMAs [dst, C, MFMAs issued since, wait states since, line]; recent: [(written regs, wait states since, line)]"""

    def __init__(self, pending=(), recent=()):
        self.pending = [list(p) for p in pending]
        self.recent = list(recent)

    def copy(self):
        return _State(self.pending, self.recent)

    def merge(self, other):
        for p in other.pending:
            if p not in self.pending:
                self.pending.append(list(p))
        for r in other.recent:
            if r not in self.recent:
                self.recent.append(r)

    def settled(self):
        return not self.pending and not self.recent


def _label_of(raw):
    m = re.match(r"^\s*(\.?L\w+):", raw)
    return m.group(1) if m else None


def _branch(op, toks):
    if (op == "s_branch" or op.startswith("s_cbranch")) and toks:
        return toks[0]
    return None


def _step(st, ln, raw, in_asm, out, via=""):
    """Advance the state over one instruction; hazards are appended to out as (key, message)."""
    p = parse(raw)
    if p is None:
        return
    op, ops, _ = p
    if op.startswith("s_nop"):
        cost = int(re.search(r"s_nop\s+(\w+)", raw).group(1), 0) + 1
    else:
        cost = 1
    for q in st.pending:
        q[3] += cost
    st.recent = [(r, w + cost, l) for (r, w, l) in st.recent if w + cost < LATE]
    if op.startswith("s_nop"):
        st.pending = [q for q in st.pending if q[3] < SETTLE]
        return
    if op.startswith("v_mfma"):
        srcs = set().union(*ops[1:]) if len(ops) > 1 else set()
        if in_asm:
            for r, w, l in st.recent:
                hit = sorted(srcs & r)
                if hit:
                    out.append(((ln, l, "late"), f"line {ln}: MFMA reads {hit[0][0]}{hit[0][1]} written {w - 1} wait states earlier (line {l}){via}"))
        for q in st.pending:
            q[2] += 1
        st.pending = [q for q in st.pending if q[2] < MIN_GAP and q[3] < SETTLE]
        if in_asm:
            c = ops[3] if len(ops) > 3 else set()
            st.pending.append([frozenset(ops[0]), frozenset(c), 0, 0, ln])
        return
    if op.startswith("s_"):
        return
    if op.startswith(_STORE) or (op.startswith("buffer_load") and re.search(r"\blds\b", raw.split(";")[0])):
        rd, wr = set().union(*ops) if ops else set(), set()
    else:
        rd = set().union(*ops[1:]) if len(ops) > 1 else set()
        wr = ops[0] if ops else set()
    for d, c, n, w, l in st.pending:
        if n >= MIN_GAP or w >= SETTLE:
            continue
        if rd & d:
            out.append(((ln, l, "read"), f"line {ln}: {op} reads {sorted(rd & d)[:2]} {n} MFMA(s) after the MFMA at line {l} that writes it{via}"))
        if wr & d:
            out.append(((ln, l, "waw"), f"line {ln}: {op} writes {sorted(wr & d)[:2]} {n} MFMA(s) after the MFMA at line {l} that writes it{via}"))
        elif wr & c:
            out.append(((ln, l, "war"), f"line {ln}: {op} writes {sorted(wr & c)[:2]} {n} MFMA(s) after the MFMA at line {l} that reads it as C{via}"))
    if op.startswith("v_"):
        if wr:
            st.recent.append((frozenset(wr), 0, ln))
        # a register rewritten by this instruction no longer holds the MFMA's (late) result as far as later READERS are concerned
        for q in st.pending:
            q[0] = q[0] - wr


def check(body):
    """Hazard messages of one kernel body (a list from kernels())."""
    labels = {}
    for i, (ln, raw, _) in enumerate(body):
        lab = _label_of(raw)
        if lab:
            labels[lab] = i
    found = {}
    st, incoming = _State(), {}
    for i, (ln, raw, in_asm) in enumerate(body):
        lab = _label_of(raw)
        if lab:
            if lab in incoming:
                st.merge(incoming.pop(lab))
            continue
        hz = []
        _step(st, ln, raw, in_asm, hz)
        for k, msg in hz:
            found.setdefault(k, msg)
        p = parse(raw)
        if p is None:
            continue
        op, _, toks = p
        tgt = _branch(op, toks)
        if tgt is not None and tgt in labels:
            if labels[tgt] > i:
                if tgt in incoming:
                    incoming[tgt].merge(st)
                else:
                    incoming[tgt] = st.copy()
            elif not st.settled():  # back edge: replay the loop head with the state of the loop's tail until it settles
                rs = st.copy()
                for ln2, raw2, asm2 in body[labels[tgt] + 1:i + 1]:
                    hz = []
                    _step(rs, ln2, raw2, asm2, hz, via=f" (via the back edge at line {ln})")
                    for k, msg in hz:
                        found.setdefault(k, msg)
                    p2 = parse(raw2)
                    if rs.settled() or (p2 is not None and p2[0] in ("s_endpgm", "s_branch", "s_setpc_b64")):
                        break
        if op in ("s_endpgm", "s_branch", "s_setpc_b64"):  # the next instruction in the listing is not reached from here
            st = _State()
    return list(found.values())


def asm_mfmas(body):
    """Line numbers of the MFMAs issued from inline asm."""
    return [ln for ln, raw, in_asm in body if in_asm and (parse(raw) or ("",))[0].startswith("v_mfma")]


def main():
    text = open(sys.argv[1]).read()
    sel = sys.argv[2] if len(sys.argv) > 2 else None
    ks = kernels(text)
    chosen = [k for k in ks if sel is None or sel == k or (k and sel in k)]
    if not chosen:
        print("kernel not found:", sel)
        sys.exit(2)
    bad = 0
    for k in chosen:
        for msg in check(ks[k]):
            print((k + ": " if len(chosen) > 1 else "") + msg)
            bad += 1
    print("hazards:", bad)


if __name__ == "__main__":
    main()
