#!/usr/bin/env python3
"""tools/disasm_cmp.py parent.s this.s — two outputs of tools/disasm.sh (LIB=<the parent's library> for the first) compared function by
function, the way notes/r16.md R16.3 says: addresses and encodings dropped, symbol names in operands and the literal of the s_add_u32 /
s_addc_u32 pair behind s_getpc_b64 masked, trailing padding ignored.  Prints every device function that is missing, new or different
(with both instruction counts) and exits 1 if the parent has one that this tree has not instruction for instruction."""
import re, sys, collections


def funcs(path):
    out = collections.OrderedDict()
    name = None
    for l in open(path):
        l = l.rstrip("\n")
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", l)
        if m:
            name = m.group(1)
            base = name
            k = 1
            while name in out:   # copies of a helper in several code objects
                k += 1
                name = "%s#%d" % (base, k)
            out[name] = []
            continue
        if name is None or "//" not in l:
            continue
        ins = l.split("//")[0].strip()
        ins = re.sub(r"<[^>]*>", "<>", ins)
        out[name].append(ins)
    for n, body in out.items():
        while body and (body[-1].startswith("s_nop") or body[-1].startswith("s_code_end") or body[-1].startswith("v_illegal")):
            body.pop()
        for i, ins in enumerate(body):
            if ins.startswith("s_getpc_b64"):
                for j in (i + 1, i + 2):
                    if j < len(body) and re.match(r"s_add(c)?_u32", body[j]):
                        body[j] = re.sub(r"(0x[0-9a-f]+|\d+)$", "LIT", body[j])
    return out


a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
print(len(a), "functions in parent,", len(b), "in this tree")
same = diff = 0
for n in a:
    if n not in b:
        print("MISSING in this tree:", n)
        diff += 1
    elif a[n] != b[n]:
        first = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        print("DIFFERS: %s  parent %d  this %d  first at %d" % (n, len(a[n]), len(b[n]), first))
        diff += 1
    else:
        same += 1
for n in b:
    if n not in a:
        print("NEW in this tree:", n)
print("same", same, "different", diff)
sys.exit(1 if diff else 0)
