"""The zero-edit launcher (launch_reference.py): a script with the reference train.py's structure - star-imports, plugin
lookups through `globals()[name]` at call time (reference train.py:167-172, 189, 208-209, 589-590), everything started
from an `if __name__ == '__main__':` block - must end up with the MI355X classes, the file untouched."""
import importlib
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launcher_rebinds_plugin_names_without_editing_the_script(tmp_path):
    pkg = tmp_path / 'models'
    pkg.mkdir()
    (pkg / '__init__.py').write_text('from models.pna import PNA\nfrom models.net3d import Net3D\n')
    (pkg / 'pna.py').write_text('class PNA:\n    origin = "reference"\n')
    (pkg / 'net3d.py').write_text('class Net3D:\n    origin = "reference"\n')
    (tmp_path / 'commons_losses.py').write_text('class NTXent:\n    origin = "reference"\nclass Other:\n    origin = "reference"\n')
    (tmp_path / 'collates.py').write_text('def contrastive_collate(b):\n    return "reference"\n')
    script = tmp_path / 'train.py'
    script.write_text(textwrap.dedent('''
        import json, sys
        from collates import *
        from models import *
        from torch.optim import *
        from commons_losses import *

        def get_trainer(args):
            return globals()[args['model3d_type']], globals()[args['loss_func']], globals()[args['optimizer']]

        def load_model(args):
            return globals()[args['model_type']]

        def train(args):
            m3, loss, opt = get_trainer(args)
            out = {'model': load_model(args).__module__, 'model3d': m3.__module__, 'loss': loss.__module__,
                   'optimizer': opt.__module__, 'collate': globals()[args['collate_function']].__module__,
                   'other': globals()['Other'].origin, 'argv': sys.argv[1:], 'name': __name__}
            print('RESULT ' + json.dumps(out))

        if __name__ == '__main__':
            train({'model_type': 'PNA', 'model3d_type': 'Net3D', 'loss_func': 'NTXent', 'optimizer': 'Adam',
                   'collate_function': 'contrastive_collate'})
    '''))
    before = script.read_text()
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'launch_reference.py'), str(script), '--config=x.yml'],
                       capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][0]
    import json
    out = json.loads(line[len('RESULT '):])
    assert out['model'] == '3dinfomax_amd.pna' and out['model3d'] == '3dinfomax_amd.net3d'
    assert out['loss'] == '3dinfomax_amd.losses' and out['collate'] == '3dinfomax_amd.graph'
    assert out['optimizer'] == '3dinfomax_amd.optim'
    assert out['other'] == 'reference'                       # names the plugin does not export stay the reference's
    assert out['argv'] == ['--config=x.yml'] and out['name'] == '__main__'
    assert script.read_text() == before
    # --keep leaves a reference class in place
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'launch_reference.py'), '--keep', 'Adam,NTXent', str(script)],
                       capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][0][len('RESULT '):])
    assert out['optimizer'].startswith('torch.optim') and out['loss'] == 'commons_losses' and out['model'] == '3dinfomax_amd.pna'


# the module layout the launcher relies on (reference train.py:50-56 star-imports; trainer/trainer.py:266-270 looks the model class
# up the same way): where each plugin name is defined, and the star-import that brings it into train.py
LAYOUT = {'models/pna.py': ['PNA'], 'models/net3d.py': ['Net3D'], 'models/pna_original.py': ['PNAOriginal', 'PNAOriginalSimple'],
          'commons/losses.py': ['NTXent', 'NTXentMultiplePositives'],
          'datasets/custom_collate.py': ['contrastive_collate', 'conformer_collate', 'graph_collate']}
LOOKUP_KEYS = ('model_type', 'model3d_type', 'loss_func', 'optimizer', 'collate_function')


def test_launcher_on_a_script_with_the_reference_layout(tmp_path):
    """The launcher's two assumptions about a script laid out like the reference's train.py - (1) it has a top-level
    `if __name__ == '__main__':` block main_block() can lift, (2) every plugin name the package exports that the script resolves
    at call time through `globals()[args.<key>]` reaches its namespace through one of its star-imports of the reference's
    modules (models, commons.losses, datasets.custom_collate, torch.optim), so rebinding that namespace is what the lookups see,
    also in trainer.trainer - checked end to end on a stand-in tree with that layout (the reference itself is not part of the
    repository)."""
    import ast
    import json

    sys.path.insert(0, ROOT)
    launcher = importlib.import_module('launch_reference')
    for rel, names in LAYOUT.items():
        path = tmp_path / rel
        path.parent.mkdir(exist_ok=True)
        (path.parent / '__init__.py').touch()
        path.write_text(''.join(f'class {n}:\n    origin = "reference"\n' if n[0].isupper() else
                                f'def {n}(batch):\n    return "reference"\n' for n in names))
    (tmp_path / 'models' / '__init__.py').write_text(
        'from models.pna import *\nfrom models.net3d import *\nfrom models.pna_original import *\n')
    (tmp_path / 'trainer').mkdir()
    (tmp_path / 'trainer' / '__init__.py').touch()
    (tmp_path / 'trainer' / 'trainer.py').write_text('from models import *\n\n\ndef model_class(name):\n    return globals()[name]\n')
    script = tmp_path / 'train.py'
    script.write_text(textwrap.dedent('''
        import argparse, json, sys
        from models import *
        from commons.losses import *
        from datasets.custom_collate import *
        from torch.optim import *
        from trainer.trainer import model_class

        def get_arguments():
            return argparse.Namespace(model_type='PNA', model3d_type='Net3D', loss_func='NTXent', optimizer='Adam',
                                      collate_function='contrastive_collate')

        def train(args):
            out = {k: globals()[getattr(args, k)].__module__ for k in %r}
            out.update({n: globals()[n].__module__ for n in %r})
            out['trainer.trainer'] = model_class(args.model_type).__module__
            print('RESULT ' + json.dumps(out))

        if __name__ == '__main__':
            args = get_arguments()
            train(args)
    ''' % (LOOKUP_KEYS, [n for names in LAYOUT.values() for n in names])))
    src = script.read_text()
    code = launcher.main_block(src, str(script))
    assert 'get_arguments' in code.co_names and 'train' in code.co_names
    tree = ast.parse(src)
    stars = [n.module for n in tree.body if isinstance(n, ast.ImportFrom) and any(a.name == '*' for a in n.names)]
    for mod in ('models', 'commons.losses', 'datasets.custom_collate', 'torch.optim'):
        assert mod in stars, (mod, stars)
    names = launcher.plugin_names()
    for n in ('PNA', 'Net3D', 'NTXent', 'NTXentMultiplePositives', 'Adam', 'contrastive_collate', 'conformer_collate',
              'graph_collate', 'PNAOriginal', 'PNAOriginalSimple'):
        assert n in names, n
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'launch_reference.py'), str(script)], capture_output=True, text=True,
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][0][len('RESULT '):])
    assert set(LOOKUP_KEYS) <= set(out)
    for k, module in out.items():
        assert module.startswith('3dinfomax_amd.'), (k, module)
    assert script.read_text() == src
