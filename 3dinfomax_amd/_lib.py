"""ctypes binding of lib3dinfomax_hip.so, DERIVED from the C ABI declared in include/infomax3d_hip.h.

The header is the single source.  It is read once per process, when this module is imported (load() and every call find the
result cached): each `typedef struct { ... } I3dName;` becomes the ctypes.Structure `Name`, each `ret i3d_name(params);` an entry
`name: (restype, argtypes)` of `_SIGNATURES`, each integer `#define I3D_*` an entry of `DEFINES`.  The reader handles exactly the
dialect the header uses and raises HipLibraryError naming the text on anything else: nothing is skipped.  One typing rule:
  int / long / long long / int64_t / uint64_t / float / double -> the ctypes scalar;  `char*` -> c_char_p;
  a pointer to a struct of the header -> POINTER(its mirror);  every other pointer (T**, `const float* const*`, void*) -> c_void_p.
The header cannot tell a host array from a device pointer, so the host arrays (int_array, ptr_array, ops._float_array) go into
c_void_p parameters as well: ctypes does not check their element type any more.

The product path has NO fallback: if the HIP library is missing or a call fails, it raises.
"""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_long, c_longlong, c_uint64, c_ulonglong, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
# test hooks (tests/test_gpu_dist.py), behind ONE flag and read ONCE, here: I3D_TESTING=1 makes I3D_TEST_PEER_SELFTEST_FAIL /
# I3D_TEST_PEER_FAIL (a rank number) and I3D_TEST_FORCE_EARLY_ALLREDUCE (1) effective; without the flag a stray variable changes nothing
_TESTING = os.environ.get('I3D_TESTING') == '1'
TEST_HOOKS = dict(peer_selftest_fail=os.environ.get('I3D_TEST_PEER_SELFTEST_FAIL') if _TESTING else None,
                  peer_fail=os.environ.get('I3D_TEST_PEER_FAIL') if _TESTING else None,
                  force_early_allreduce=_TESTING and os.environ.get('I3D_TEST_FORCE_EARLY_ALLREDUCE') == '1',
                  verbose_selftest=_TESTING and bool(os.environ.get('I3D_DEBUG_SELFTEST')))
LIB_PATH = os.environ.get('I3D_LIB_PATH') or os.path.join(HERE, 'lib', 'lib3dinfomax_hip.so')      # (override: kernel probes of tools/probes)
HEADER_PATH = os.path.join(os.path.dirname(HERE), 'include', 'infomax3d_hip.h')


class HipLibraryError(RuntimeError):
    pass


# ---- the header reader ---------------------------------------------------------------------------------------------------
_SCALARS = {'int': c_int, 'long': c_long, 'long long': c_longlong, 'int64_t': c_int64, 'uint64_t': c_uint64,
            'unsigned long long': c_ulonglong, 'float': c_float, 'double': c_double}
_POINTEES = ('void', 'char', 'unsigned char')      # besides the scalars and the header's structs
_DECL = re.compile(r'(?P<base>[A-Za-z_]\w*(?: [A-Za-z_]\w*){0,2}?)(?P<ptr>(?: \*)*) (?P<name>[A-Za-z_]\w*)')
_STATEMENT = re.compile(r'\s*(?:typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)|(?P<decl>[^;{}()]+)\((?P<params>[^;{}()]*)\))\s*;')
_DECLARATOR = re.compile(r'(?P<head>[^\[\]]*)(?P<dims>(?:\[[^\]]*\]\s*)*)')
_FN_MEMBER = re.compile(r'(?P<ret>[^()]+)\(\s*\*\s*(?P<name>\w+)\s*\)\s*\((?P<params>[^()]*)\)')


def _fail(what, text):
    raise HipLibraryError(f'include/infomax3d_hip.h: {what}: {" ".join(text.split())!r}')


def _split(text):
    """`const float* const* tables` -> ('float', 2, 'tables')"""
    m = _DECL.fullmatch(' '.join(t for t in re.findall(r'\w+|\S', text) if t != 'const'))
    if not m or m['name'] in _SCALARS or m['name'] in _POINTEES:
        _fail('not `type name` (an unnamed parameter?)', text)
    return m['base'], m['ptr'].count('*'), m['name']


def _declaration(text, structs):
    """`const float* const* tables` -> ('tables', c_void_p): the typing rule of the module docstring"""
    base, ptr, name = _split(text)
    if base not in _SCALARS and base not in structs and not (ptr and base in _POINTEES):
        _fail(f'unknown type {base!r}', text)
    if not ptr:
        return name, _SCALARS.get(base) or structs[base]
    if ptr == 1 and base == 'char':
        return name, c_char_p
    return name, POINTER(structs[base]) if ptr == 1 and base in structs else c_void_p


def _parameters(text, structs):
    return [] if text.strip() == 'void' else [_declaration(p, structs)[1] for p in text.split(',')]


def _bound(expr, defines, text):
    """an array bound: an integer expression over the header's defines, e.g. `I3D_MAX_EXTRA_FC + 1`"""
    try:
        value = re.sub(r'[A-Za-z_]\w*', lambda m: str(defines[m[0]]), expr)
        if not re.fullmatch(r'[\d\s+\-*()]+', value):
            raise ValueError(value)
        n = eval(value, {'__builtins__': {}})      # digits, + - * and parentheses only
    except (KeyError, ValueError, SyntaxError):
        _fail(f'array bound [{expr.strip()}] does not evaluate', text)
    return n if n > 0 else _fail(f'array bound [{expr.strip()}] is not positive', text)


def _fields(body, defines, structs):
    """the members of one struct, in declaration order: `int ldw, N, K, trans;`, `I3dFcParams pre[A][B + 1];`, callbacks"""
    fields = []
    for member in filter(str.strip, body.split(';')):
        fn = _FN_MEMBER.fullmatch(member.strip())
        if fn:
            ret = _declaration(f"{fn['ret']} {fn['name']}", structs)[1]
            fields.append((fn['name'], ctypes.CFUNCTYPE(ret, *_parameters(fn['params'], structs))))
            continue
        base = None
        for declarator in member.split(','):      # `int n_groups, group_start[32]`, `int64_t *src, *dst`: one type, several declarators
            d = _DECLARATOR.fullmatch(declarator) or _fail('not a declarator', member)
            head = d['head'] if base is None else f"{base} {d['head']}"
            base = base or _split(head)[0]
            name, t = _declaration(head, structs)
            for dim in reversed(re.findall(r'\[([^\]]*)\]', d['dims'])):      # a[2][3]: two arrays of three
                t = t * _bound(dim, defines, member)
            fields.append((name, t))
    return fields


def parse_header(text):
    """(defines, structs, signatures) of a header in the dialect of include/infomax3d_hip.h; HipLibraryError on anything else"""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    defines = {m[1]: int(m[2] or m[3])
               for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(I3D_\w+)[ \t]+(?:(-?\d+)|\((-?\d+)\))[ \t]*$', text, re.M)}
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', '', text)
    if n_extern:
        text, brace, rest = text.rpartition('}')
        if not brace or rest.strip():
            _fail('the brace of extern "C" does not close the file', rest or text[-80:])
    structs, signatures, pos = {}, {}, 0
    while text[pos:].strip():
        m = _STATEMENT.match(text, pos)
        if not m:
            end = re.compile(r'(?:[^;{}]|\{[^{}]*(?:\{[^{}]*\}[^{}]*)*\})*').match(text, pos).end()      # its `;` outside braces
            _fail('neither a prototype nor a `typedef struct { ... } Name;` of plain members', text[pos:end])
        if m['struct'] in structs or (m['decl'] and _split(m['decl'])[2] in signatures):
            _fail('declared twice', m[0])
        if m['struct']:
            structs[m['struct']] = type(m['struct'].removeprefix('I3d'), (ctypes.Structure,),
                                        {'_fields_': _fields(m['body'], defines, structs)})
        else:
            name, restype = _declaration(m['decl'], structs)
            signatures[name] = (restype, _parameters(m['params'], structs))
        pos = m.end()
    return defines, {s.__name__: s for s in structs.values()}, signatures


with open(HEADER_PATH) as _f:
    DEFINES, STRUCTS, _SIGNATURES = parse_header(_f.read())
# the argument structs by the names the package uses: BnTail, FcArgs, EdgeFcArgs, GroupedFcArgs, PnaLayerArgs, Net3dEdgeArgs, FcParams,
# PnaModel, PnaBatch, BnEvalAff, CopyBlock, PanelPack, TowerLayerArgs, NodeDropView, Collectives, WgradProblem, WgradOutput
globals().update(STRUCTS)
ALL_GATHER_F32, ALL_REDUCE_F64 = (dict(STRUCTS['Collectives']._fields_)[k] for k in ('all_gather_f32', 'all_reduce_f64'))


def _codes(prefix):
    """{'leakyrelu': 4, ...} from the header's `#define I3D_ACT_LEAKY_RELU 4`, ..."""
    return {k[len(prefix):].replace('_', '').lower(): v for k, v in DEFINES.items() if k.startswith(prefix)}


ACT = {None: DEFINES['I3D_ACT_NONE'], **_codes('I3D_ACT_')}
AGG = _codes('I3D_AGG_')
SCALER = _codes('I3D_SCALE_')
NOISED = _codes('I3D_NOISED_')      # the noising kinds of i3d_noised_graph_build
NOT_TAKEN = DEFINES['I3D_NOT_TAKEN']      # a valid call outside what the entry point's kernels cover; nothing was launched


def array_len(struct, member):
    """the declared length of an array member, e.g. array_len(GroupedFcArgs, 'coef'): the header's bound, not a copy of it"""
    return dict(struct._fields_)[member]._length_


def declared_symbols():
    """Function names declared in include/infomax3d_hip.h."""
    return sorted(_SIGNATURES)


_lib = None


def load():
    """Load the C-ABI library (once) and attach argtypes.  Raises HipLibraryError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    # I3D_MATMUL_PRECISION=bf16: the trainer of the reference has no knob for it (ops.set_matmul_precision otherwise)
    prec = os.environ.get('I3D_MATMUL_PRECISION', 'fp32').lower()
    if prec not in ('fp32', 'bf16'):
        raise HipLibraryError(f'I3D_MATMUL_PRECISION={prec!r}: fp32 or bf16')
    lib.i3d_set_matmul_precision(int(prec == 'bf16'))
    _lib = lib
    return lib


def check(rc, name):
    if rc != 0:
        msg = load().i3d_last_error()
        raise HipLibraryError(f'{name} failed (rc={rc}): {msg.decode() if msg else ""}')


def int_array(values):
    return (c_int * len(values))(*values)


def ptr_array(ptrs):
    return (c_void_p * len(ptrs))(*ptrs)
