"""The one parser of the public headers (include/*.h) that the binding tests share: prototypes as the kind codes of `_C`'s signature
tables, the field names of a struct in order, and the integer #defines.  Helpers only, no tests."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')


def _code(header):
    """the text of include/<header> without its comments"""
    txt = open(os.path.join(INCLUDE, header)).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    return re.sub(r'//.*$', ' ', txt, flags=re.M)


def kind(decl, is_return=False):
    """kind code of a C type (a parameter declaration with or without its name)"""
    if '*' in decl:
        return 's' if is_return and 'char' in decl else 'p'
    words = decl.replace('const', ' ').split()
    return {'int': 'i', 'int32_t': 'i', 'int64_t': 'l', 'float': 'f', 'double': 'd', 'void': 'v'}[words[0]]


def prototypes(header):
    """{name: (return kind, parameter kinds)} of every vqn_* function the header declares, in its order"""
    txt = re.sub(r'^\s*#.*$', ' ', _code(header), flags=re.M)
    out = {}
    for ret, name, params in re.findall(r'([\w\s*]+?)\s*\b(vqn_\w+)\s*\(([^)]*)\)\s*;', txt):
        params = [p for p in params.split(',') if p.strip() not in ('', 'void')]
        out[name] = (kind(ret, True), ''.join(kind(p) for p in params))
    return out


def struct_fields(header, struct):
    """the field names of `struct <struct> { ... }`, in order (scalar and array fields of one-word types)"""
    body = re.search(r'\bstruct\s+%s\s*\{([^}]*)\}' % struct, _code(header)).group(1)
    names = []
    for decl in body.split(';'):
        if decl.strip():
            fields = decl.split(None, 1)[1]                      # after the type
            names += [re.sub(r'\[.*?\]|[\s*]', '', f) for f in fields.split(',')]
    return names


def defines(header):
    """{NAME: value} of the header's `#define NAME integer` lines"""
    return {name: int(value, 0) for name, value in re.findall(r'^\s*#\s*define\s+(\w+)\s+(-?\w+)\s*$', _code(header), flags=re.M)
            if re.fullmatch(r'-?(0[xX][0-9a-fA-F]+|\d+)', value)}


def function_headers():
    """the files of include/ that declare at least one vqn_* function"""
    return sorted(h for h in os.listdir(INCLUDE) if h.endswith('.h') and prototypes(h))
