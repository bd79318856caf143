"""The contrastive metrics on offset, collapsed and aligned inputs (fixture tests/golden/gen_golden_metrics_edges.py, generated from the
reference's own trainer/metrics.py in fp32 and in fp64): the fp64 oracle against the reference's fp64 values, and the two conditions
on the fixture's inputs that the GPU test (tests/test_gpu_metrics_edges.py) relies on."""
import functools
import math

import numpy as np
import pytest
import torch

from helpers import load
from oracle import metrics_oracle as MO

import gen_golden_metrics_edges as GE
from test_metrics import _close


@functools.lru_cache(maxsize=None)
def edge_cases():
    """-> per case {tag, base, family, z1, z2 (fp32 numpy, from the shared builder), v32 / v64 {name: value}}; built once, not to be
    modified"""
    z = load('metrics_edges.npz')
    bases = GE.fixture_bases(z)
    cases = []
    for i, (base, family) in enumerate(GE.CASES):
        z1, z2 = GE.build(bases[base], family)
        z1.setflags(write=False), z2.setflags(write=False)
        cases.append({'tag': GE.TAGS[i], 'base': base, 'family': family, 'z1': z1, 'z2': z2, 'checks': z['checks'][i],
                      'v32': dict(zip(GE.NAMES, z['values'][i, :, 0])), 'v64': dict(zip(GE.NAMES, z['values'][i, :, 1]))})
    return cases


def test_cases_are_the_ones_the_fixture_was_made_for():
    tags = set(GE.TAGS)
    assert len(tags) == len(GE.CASES) == 20
    assert {f'96x64_{f}' for f in GE.FAMILIES} <= tags
    for shape in ('2x16', '257x64', '40x300', '32x64+32'):
        assert {f'{shape}_{f}' for f in ('offset30', 'collapsed', 'aligned_off')} <= tags


@pytest.mark.parametrize('idx', range(len(GE.CASES)), ids=GE.TAGS)
def test_builder_reproduces_the_stored_checks(idx):
    c = edge_cases()[idx]
    B1, D, extra, _ = GE.BASES[c['base']]
    assert c['z1'].shape == (B1, D) and c['z2'].shape == (B1 + extra, D) and c['z1'].dtype == np.float32 and c['z2'].dtype == np.float32
    assert np.array_equal(GE.checks(c['z1'], c['z2']), c['checks'])          # bitwise: the builder is exact fp32 arithmetic
    assert np.array_equal(GE.base_arrays(c['base'])['n1'], load('metrics_edges.npz')[f'base/{c["base"]}/n1'])


@pytest.mark.parametrize('idx', range(len(GE.CASES)), ids=GE.TAGS)
def test_inputs_keep_clear_of_the_threshold_and_of_underflow(idx):
    c = edge_cases()[idx]
    margin = GE.rate_margin(c['z1'], c['z2'])
    pots = GE.log_potentials(c['z1'], c['z2'])
    print(f'{c["tag"]}: smallest |(cos + 1) / 2 - threshold| {margin:.3e}, log potentials {pots[0]:.4f} {pots[1]:.4f}')
    assert margin > 1e-4
    assert min(pots) > -80.0


@pytest.mark.parametrize('idx', range(len(GE.CASES)), ids=GE.TAGS)
def test_oracle_in_fp64_reproduces_the_reference_fp64_values(idx):
    c = edge_cases()[idx]
    got = MO.all_metrics(torch.from_numpy(c['z1']).double(), torch.from_numpy(c['z2']).double())
    for name in GE.NAMES:
        want = float(c['v64'][name])
        if math.isnan(want):
            assert math.isnan(got[name]), (c['tag'], name, got[name])
        else:
            assert _close(got[name], want), (c['tag'], name, got[name], want)
    if c['family'] == 'zero_row':
        assert {n for n in GE.NAMES if math.isnan(c['v64'][n])} == {n for n in GE.NAMES if math.isnan(c['v32'][n])} != set()
