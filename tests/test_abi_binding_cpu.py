"""The ctypes binding is derived from include/infomax3d_hip.h (3dinfomax_amd/_lib.py): exact types of one prototype and one struct
member per construct of the header's dialect, the reader's refusal of everything outside that dialect, one parse per process,
and every Python constant that names a header #define.  No GPU is needed."""
import builtins
import ctypes
import importlib
import importlib.util
import re
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_uint64, c_void_p

import pytest

L = importlib.import_module('3dinfomax_amd._lib')
ops = importlib.import_module('3dinfomax_amd.ops')
dataset = importlib.import_module('3dinfomax_amd.dataset')

P = c_void_p
PROTOTYPES = {
    # int64_t*, const float* const*
    'i3d_embedding_sum_fwd': (c_int, [P, P, c_int, c_int, P, c_int, P, P]),
    # long long*
    'i3d_act_stats_fwd_counted': (c_int, [P, c_int, c_int, c_int, P, c_float, c_float, P, P, P, P, P, P, P, P]),
    # 64-bit unsigned and float scalars
    'i3d_noised_graph_build': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int, c_float, c_uint64, c_uint64] + [P] * 12),
    # double scalars
    'i3d_adam_step': (c_int, [P, c_int, P, c_int] + [c_double] * 7 + [P]),
    # returns const char*, (void) parameter list
    'i3d_last_error': (c_char_p, []),
    # char*
    'i3d_rccl_unique_id': (c_int, [c_char_p]),
    # returns long long
    'i3d_peer_sequence': (c_longlong, [P]),
    # returns long, struct pointer
    'i3d_tower_layer_saved_floats': (c_long, [POINTER(L.TowerLayerArgs)]),
    # two struct pointers, void* const*, void**
    'i3d_pna_model_fwd': (c_int, [POINTER(L.PnaModel), POINTER(L.PnaBatch), P, P, P, P, P, P, P, P]),
    # returns long, two int parameters
    'i3d_colreduce_workspace_bytes': (c_long, [c_int, c_int]),
}


@pytest.mark.parametrize('name', sorted(PROTOTYPES))
def test_prototype_types_are_exactly_the_headers(name):
    restype, argtypes = L._SIGNATURES[name]
    assert (restype, list(argtypes)) == PROTOTYPES[name]


def _field(struct, name):
    return dict(struct._fields_)[name]


def test_struct_members_are_exactly_the_headers():
    # `int ldw, N, K, trans;` between two pointers
    assert L.PanelPack._fields_ == [('W', P), ('ldw', c_int), ('N', c_int), ('K', c_int), ('trans', c_int), ('packed', P)]
    assert ctypes.sizeof(L.PanelPack) == 32
    # bounds that are expressions over the header's defines, one and two dimensions
    assert _field(L.PnaLayerArgs, 'aff') is c_void_p * 4
    assert _field(L.PnaModel, 'pre') is (L.FcParams * 4) * 16
    assert _field(L.PnaModel, 'head') is L.FcParams * 4
    assert _field(L.GroupedFcArgs, 'group_start') is c_int * 32 and _field(L.GroupedFcArgs, 'coef') is c_float * 128
    assert L.array_len(L.GroupedFcArgs, 'group_start') == 32 and L.array_len(L.GroupedFcArgs, 'coef') == 128
    # `int n_aggregators, aggregators[8];`: an array behind a scalar in one declaration
    names = [f[0] for f in L.PnaModel._fields_]
    assert names[names.index('n_aggregators') + 1] == 'aggregators' and _field(L.PnaModel, 'aggregators') is c_int * 8
    # a struct of the header by value, and in an array
    assert _field(L.FcArgs, 'tail') is L.BnTail
    assert _field(L.PnaLayerArgs, 'pre') is L.FcArgs * 3
    # `int64_t *src, *dst, ...;`: the star belongs to the declarator
    assert all(_field(L.NodeDropView, k) is P for k in ('keep', 'src', 'bond_feat', 'in_ptr', 'deg_rows'))
    assert _field(L.NodeDropView, 'rows') is c_int


def test_collectives_callbacks_are_cfunctypes_of_the_headers_parameter_lists():
    gather, reduce_ = _field(L.Collectives, 'all_gather_f32'), _field(L.Collectives, 'all_reduce_f64')
    assert L.ALL_GATHER_F32 is gather and L.ALL_REDUCE_F64 is reduce_
    for cb, argtypes in ((gather, (P, P, P, c_long, P)), (reduce_, (P, P, c_long, P))):
        assert issubclass(cb, ctypes._CFuncPtr) and cb._restype_ is c_int and tuple(cb._argtypes_) == argtypes
    assert [f[0] for f in L.Collectives._fields_] == ['world', 'all_gather_f32', 'all_reduce_f64', 'user', 'scratch', 'scratch_bytes']


def test_every_struct_and_prototype_of_the_header_is_bound():
    text = re.sub(r'/\*.*?\*/', '', open(L.HEADER_PATH).read(), flags=re.S)
    assert sorted(L.STRUCTS) == sorted(n[3:] for n in re.findall(r'\}\s*(I3d\w+)\s*;', text)) and len(L.STRUCTS) == 17
    assert L.declared_symbols() == sorted(set(re.findall(r'\b(i3d_[a-z0-9_]+)\s*\(', text))) == sorted(L._SIGNATURES)
    for name, struct in L.STRUCTS.items():
        assert getattr(L, name) is struct and struct.__name__ == name


REFUSED = {
    'unknown type': ('int i3d_f(const float* x, size_t n);', 'size_t n'),
    'unknown pointee': ('int i3d_f(hipStream_t* s);', 'hipStream_t* s'),
    'unnamed parameter': ('int i3d_f(const float* x, int);', 'int'),
    'unnamed pointer parameter': ('int i3d_f(const float*, int n);', 'const float*'),
    'union': ('typedef union { int i; float f; } I3dU;', 'union'),
    'union member': ('typedef struct { int n; union { int i; float f; } u; } I3dS;', 'union'),
    'undefined macro in a bound': ('#define I3D_A 2\ntypedef struct { int a[I3D_A]; float b[I3D_B + 1]; } I3dS;', 'I3D_B + 1'),
    'bound that is no integer expression': ('typedef struct { int a[sizeof(int)]; } I3dS;', 'sizeof(int)'),
    'variable': ('int i3d_f(int n);\nint i3d_counter;', 'int i3d_counter'),
    'function body': ('static inline int i3d_f(int n) { return n; }', 'static inline int i3d_f(int n)'),
    'enum': ('enum I3dE { I3D_X, I3D_Y };\nint i3d_f(int n);', 'enum I3dE'),
    'prototype declared twice': ('int i3d_f(int n);\nint i3d_g(void);\nlong i3d_f(long n);', 'long i3d_f(long n)'),
    'by-value struct never declared': ('int i3d_f(I3dMissing m);', 'I3dMissing m'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_reader_refuses_what_is_outside_the_dialect_and_names_it(case):
    text, offending = REFUSED[case]
    with pytest.raises(L.HipLibraryError) as e:
        L.parse_header(text)
    assert offending in str(e.value)


def test_reader_on_a_snippet_of_every_accepted_form():
    defines, structs, sigs = L.parse_header('''
        #ifndef GUARD_H
        #define GUARD_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define I3D_N 3      /* a comment */
        #define I3D_NEG (-2) // another
        #define I3D_NAME "text"
        typedef struct { const float* w; int a, b[I3D_N + 1]; } I3dInner;
        typedef struct { I3dInner one; I3dInner grid[2][I3D_N]; long (*cb)(void* user, const I3dInner* p, double v); } I3dOuter;
        long long i3d_f(const I3dOuter* o /* host */, I3dInner** list, const char* name, uint64_t seed, void* stream);
        const char* i3d_g(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    ''')
    assert defines == {'I3D_N': 3, 'I3D_NEG': -2}
    inner, outer = structs['Inner'], structs['Outer']
    assert inner._fields_ == [('w', P), ('a', c_int), ('b', c_int * 4)]
    assert outer._fields_[:2] == [('one', inner), ('grid', (inner * 3) * 2)]
    cb = _field(outer, 'cb')
    assert cb._restype_ is c_long and tuple(cb._argtypes_) == (P, POINTER(inner), c_double)
    assert sigs == {'i3d_f': (c_longlong, [POINTER(outer), P, c_char_p, c_uint64, P]), 'i3d_g': (c_char_p, [])}


def test_header_is_read_once_per_process_and_never_by_load_or_a_call(monkeypatch):
    reads, real_open = [], builtins.open

    def counting_open(path, *a, **k):
        if path == L.HEADER_PATH:
            reads.append(path)
        return real_open(path, *a, **k)
    monkeypatch.setattr(builtins, 'open', counting_open)
    sigs = L._SIGNATURES
    L.load(), L.load()
    assert L.declared_symbols() == sorted(sigs) and L._SIGNATURES is sigs
    assert reads == []      # this process read it when the module was imported
    # what a fresh process does, without starting one: the module's code run once more, under another name
    spec = importlib.util.spec_from_file_location('_lib_second_import', L.__file__)
    second = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(second)
    second.declared_symbols(), second.declared_symbols()
    assert reads == [L.HEADER_PATH] and sorted(second._SIGNATURES) == sorted(sigs)


def _header_defines():
    text = open(L.HEADER_PATH).read()
    return {k: int(v.strip('()')) for k, v in re.findall(r'^#define (I3D_\w+) (\(?-?\d+\)?)', text, flags=re.M)}


def test_python_constants_are_the_headers_defines():
    d = _header_defines()
    assert L.DEFINES == d and d['I3D_ERR_INVALID'] == -1
    assert L.NOT_TAKEN == d['I3D_NOT_TAKEN']
    assert ops.GEOMOL_PARTIAL_FLOATS == d['I3D_GEOMOL_PARTIAL_FLOATS']
    assert L.ACT == {None: d['I3D_ACT_NONE'], 'none': d['I3D_ACT_NONE'], 'relu': d['I3D_ACT_RELU'], 'silu': d['I3D_ACT_SILU'],
                     'sigmoid': d['I3D_ACT_SIGMOID'], 'leakyrelu': d['I3D_ACT_LEAKY_RELU'], 'tanh': d['I3D_ACT_TANH'],
                     'elu': d['I3D_ACT_ELU'], 'selu': d['I3D_ACT_SELU'], 'softplus': d['I3D_ACT_SOFTPLUS']}
    assert L.AGG == {'mean': d['I3D_AGG_MEAN'], 'sum': d['I3D_AGG_SUM'], 'max': d['I3D_AGG_MAX'], 'min': d['I3D_AGG_MIN'],
                     'std': d['I3D_AGG_STD'], 'var': d['I3D_AGG_VAR']}
    assert L.SCALER == {'identity': d['I3D_SCALE_IDENTITY'], 'amplification': d['I3D_SCALE_AMPLIFICATION'],
                        'attenuation': d['I3D_SCALE_ATTENUATION']}
    assert (ops.WGRAD_PLAIN, ops.WGRAD_BN, ops.WGRAD_COMBINE) == (d['I3D_WGRAD_PLAIN'], d['I3D_WGRAD_BN'], d['I3D_WGRAD_COMBINE'])
    assert dataset.NOISED_MODES == {'distances': d['I3D_NOISED_DISTANCES'], 'coordinates': d['I3D_NOISED_COORDINATES']}
    assert ops.ACT is L.ACT and ops.AGG is L.AGG and ops.SCALER is L.SCALER
