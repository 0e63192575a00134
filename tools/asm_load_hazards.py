"""Registers of loads in flight, checked in a kernel's assembly (`hipcc -O3 -S --cuda-device-only --offload-arch=gfx950 csrc/<file>.hip -o FILE.s`).
Kernels that issue global loads from inline asm and wait for them by counted `s_waitcnt vmcnt(N)` hide those loads from the compiler: a destination
register that no later statement names is free for it to reuse while the load is still in flight, and a late return then overwrites the new value.
This walks every path through each kernel whose name contains NAME (basic blocks and branches from the labels), keeps the in-order queue of outstanding
VMEM operations as the state (loads, LDS-DMA loads and stores all count; a `vmcnt(N)` leaves the youngest N), and reports every instruction other than a later load that writes a VGPR which an outstanding load will still
write, and the loads still outstanding at s_endpgm.  `s_cbranch_execnz` is taken as a jump: a running wave has a lane.  Path conditions are not
evaluated, so a report on a path that cannot run is possible; none is a pass.  Exit status 1 if anything is reported.
usage: asm_load_hazards.py FILE.s [NAME]      (DESIGN 7c''': k_sconv_b1s2)"""
import re,sys
def regs(tok):
    m=re.match(r'v\[(\d+):(\d+)\]$',tok)
    if m: return frozenset(range(int(m.group(1)),int(m.group(2))+1))
    m=re.match(r'v(\d+)$',tok)
    return frozenset({int(m.group(1))}) if m else frozenset()
def kernels(path):
    cur=None; out={}
    for line in open(path):
        m=re.match(r'^(_Z\w+):',line)
        if m: cur=m.group(1); out[cur]=[]; continue
        if cur and line.startswith('.Lfunc_end'): cur=None
        if cur is not None: out[cur].append(line)
    return out
def analyse(name, lines):
    blocks=[['entry',[]]]
    for ln,line in enumerate(lines):
        l=line.split(';')[0].strip()
        if not l: continue
        m=re.match(r'^(\.LBB\w+):',l)
        if m: blocks.append([m.group(1),[]]); continue
        if l.startswith('.') : continue
        blocks[-1][1].append((ln,l))
    idx={b[0]:i for i,b in enumerate(blocks)}
    seen=set(); work=[(0,())]; haz=set(); endout=0; maxq=0
    while work:
        bi,q=work.pop()
        if (bi,q) in seen: continue
        seen.add((bi,q)); q=list(q); nxt=[]; fall=True
        for ln,l in blocks[bi][1]:
            toks=l.replace(',',' ').split(); op=toks[0]
            if op=='s_waitcnt':
                m=re.search(r'vmcnt\((\d+)\)',l)
                if m: q=q[max(0,len(q)-int(m.group(1))):] if int(m.group(1)) else []
                continue
            if op=='s_endpgm':
                endout=max(endout,len([1 for dst,_ in q if dst])); fall=False; break   # (stores may be in flight at the end, loads into registers not)
            if op=='s_branch': nxt.append(idx[toks[1]]); fall=False; break
            if op=='s_cbranch_execnz': nxt.append(idx[toks[1]]); fall=False; break   # a wave that runs has a lane: the compiler's way of writing a jump out of a loop
            if op.startswith('s_cbranch'): nxt.append(idx[toks[1]]); continue
            if op.startswith(('global_store', 'buffer_store', 'global_load_lds')):   # they count in vmcnt (gfx9: stores too) and write no VGPR
                q.append((frozenset(), ln)); maxq = max(maxq, len(q)); continue
            if op.startswith(('ds_write', 's_', 'v_cmp', 'v_readfirstlane', 'v_readlane')): continue
            d=regs(toks[1]) if len(toks)>1 else frozenset()
            if not op.startswith('global_load'):                       # (a later VMEM load into the same register returns later: loads return in order)
                for dst,where in q:
                    if d & dst: haz.add((ln,l,where))
            if op.startswith('global_load'): q.append((d,ln)); maxq=max(maxq,len(q))
        if fall and bi+1<len(blocks): nxt.append(bi+1)
        for n in nxt: work.append((n,tuple(q)))
    for h in sorted(haz)[:12]: print('  HAZARD: line %d `%s` writes a destination of the load at line %d'%h)
    print('%s: %d blocks, %d (block, queue) states, max outstanding %d, hazards %d, outstanding at s_endpgm %d'%(name,len(blocks),len(seen),maxq,len(haz),endout))
    return len(haz) + endout
if __name__ == "__main__":
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    bad = 0
    for name, lines in kernels(sys.argv[1]).items():
        if want in name:
            bad += analyse(name, lines)
    sys.exit(1 if bad else 0)
