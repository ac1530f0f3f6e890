import re, sys, difflib
def funcs(path):
    out, cur, name = {}, None, None
    for ln in open(path):
        m = re.match(r'^(_ZN3c3h\S+):\s', ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if ln.startswith('.Lfunc_end'):
                out[name] = cur; cur = None
                continue
            s = ln.split(';')[0].rstrip() if not ln.strip().startswith(';') else ''
            if s.strip() and not s.strip().startswith('.'):
                cur.append(s)
            elif re.match(r'^\.LBB', s): cur.append(s)
    return out
def norm(name, body):
    # symbol-name differences: mangled kernel names inside labels / relocations
    short = re.sub(r'I?NS0_9PtsXyzrgbEEEv', '', name)
    return [re.sub(r'_ZN3c3h\S+', 'SYM', re.sub(r'\.LBB\d+_', '.LBB_', l)) for l in body]
a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
def key(n):
    return (n.replace('INS0_9PtsXyzrgbEEEv', 'E'), 'PtsPc2' in n)
A = {key(n)[0]: (n, v) for n, v in a.items()}
for n, v in b.items():
    k, pc2 = key(n)
    if pc2: continue
    if k not in A:
        print('NEW', n); continue
    pa = norm(*A[k]); pb = norm(n, v)
    d = list(difflib.unified_diff(pa, pb, 'parent', 'tree', lineterm='', n=1))
    print('%-28s parent %5d instr, tree %5d instr: %s' % (k, len(pa), len(pb), 'IDENTICAL' if not d else '%d diff lines' % len(d)))
    for l in d[:200]: print('   ', l)
