"""BYOL pre-training wrapper: drop-in for reference trainer/byol_wrapper.py:12-53 (configs/byol.yml: model_type and model3d_type
'BYOLwrapper' around PNA and Net3D, trainer 'byol', loss_func CosineSimilarityLoss).

A student network with a predictor head, and a teacher that is a copy of the student whose parameters follow it as a moving
average (`ma_teacher_update`, called by the reference's BYOLTrainer.after_optim_step, trainer/byol_trainer.py:22).  The reference
forms `t * d + s * (1 - d)` per parameter in Python - three launches and a new storage for every tensor.  Here all (student, teacher)
pairs are ONE launch of csrc/ema.hip over a device-resident chunk table built once (the pattern of optim._NativeTable), in place:
the teacher's storages never move, and the values are the reference's bit for bit (same three roundings, no fused multiply-add).
"""
import copy
import struct

import torch
from torch import nn

from . import tape
from .graph import as_batched_graph


class _EmaTable:
    """device-resident chunk table of csrc/ema.hip for one list of (teacher, student) parameter pairs; pairs the kernel does not
    take (not contiguous fp32 on the launch device) are kept aside for the torch expression"""

    def __init__(self, teacher, student):
        from . import _lib
        self.t_ptrs = [p.data_ptr() for p in teacher]
        self.s_ptrs = [p.data_ptr() for p in student]
        self.fallback = []
        self.n_chunks, self.table = 0, None
        dev = next((t.device for t in teacher if t.is_cuda), None)
        if dev is None or dev.index != torch.cuda.current_device():      # (the launch goes to the current device's stream)
            self.fallback = list(zip(teacher, student))
            return
        L = _lib.load()
        ch, rec = L.i3d_ema_chunk_elems(), L.i3d_ema_chunk_bytes()
        assert rec == 24
        buf = bytearray()
        for t, s in zip(teacher, student):
            if not (t.device == dev and s.device == dev and t.dtype == torch.float32 and s.dtype == torch.float32
                    and t.is_contiguous() and s.is_contiguous() and t.shape == s.shape):
                self.fallback.append((t, s))
                continue
            n = t.numel()
            for o in range(0, n, ch):
                buf += struct.pack('<QQiI', t.data_ptr() + 4 * o, s.data_ptr() + 4 * o, min(ch, n - o), 0)
        self.n_chunks = len(buf) // rec
        if self.n_chunks:
            self.table = torch.frombuffer(buf, dtype=torch.uint8).clone().to(dev)

    def valid_for(self, teacher, student):
        # a parameter whose storage moved (.to(), checkpoint surgery): the table points at the old memory
        return [p.data_ptr() for p in teacher] == self.t_ptrs and [p.data_ptr() for p in student] == self.s_ptrs


class BYOLwrapper(nn.Module):
    """reference trainer/byol_wrapper.py:12-53: `student` (with gradients) -> `predictor`; `teacher`, a copy without gradients"""

    def __init__(self, model_type, model_parameters, predictor_layers=1, predictor_hidden_size=256, predictor_batchnorm=False,
                 metric_dim=256, ma_decay=0.99, **kwargs):
        super().__init__()
        self.student = _model_class(model_type)(**model_parameters, **kwargs)
        # before any forward: nothing the student caches per call (layers.FCLayer.hot, the pointer descriptions of pna_native /
        # layer_native, the tape's per-model state) exists yet, so the copy starts without any of it
        self.teacher = copy.deepcopy(self.student)
        self.predictor_layers = predictor_layers
        if predictor_layers > 0:
            from .layers import MLP
            self.predictor = MLP(in_dim=model_parameters['target_dim'], hidden_size=predictor_hidden_size,
                                 mid_batch_norm=predictor_batchnorm, out_dim=metric_dim, layers=predictor_layers)
        self.ma_decay = ma_decay
        for p in self.teacher.parameters():
            p.requires_grad = False

    def ma_teacher_update(self):
        """teacher = teacher * ma_decay + student * (1 - ma_decay) for every parameter (not the buffers), in place"""
        d = float(self.ma_decay)
        teacher, student = tape._param_list(self.teacher), tape._param_list(self.student)
        tab = self.__dict__.get('_i3d_ema')
        if tab is None or not tab.valid_for(teacher, student):
            tab = self.__dict__['_i3d_ema'] = _EmaTable(teacher, student)
        if tab.n_chunks:
            from . import _lib, ops
            # torch turns the Python scalars d and 1 - d into fp32 once each; so does the conversion to c_float here
            _lib.check(_lib.load().i3d_ema_update(tab.table.data_ptr(), tab.n_chunks, d, 1.0 - d, ops._stream()), 'i3d_ema_update')
        if tab.fallback:
            with torch.no_grad():
                for t, s in tab.fallback:
                    # the product as a tensor of its own: add_(s, alpha=1 - d) is one fused multiply-add per element in torch's
                    # CPU kernel - two roundings where the reference's expression has three
                    t.mul_(d).add_(s * (1.0 - d))

    def forward(self, graph):
        g = as_batched_graph(graph)
        g.index()                       # built once, shared by both copies
        # the models overwrite ndata['feat'] / edata: the teacher gets frames of its own around the same tensors and kernel index
        # (the reference deep-copies the whole graph, trainer/byol_wrapper.py:43)
        graph_t = g.local_copy()
        projection_s = self.student(g)
        prediction_s = self.predictor(projection_s) if self.predictor_layers > 0 else projection_s
        with torch.no_grad():
            projection_t = self.teacher(graph_t)
        return prediction_s, projection_t


def _model_class(model_type):
    """the package's model class of that name (the reference looks `model_type` up among its own `models`)"""
    import importlib
    pkg = importlib.import_module(__package__)
    cls = getattr(pkg, model_type, None) if model_type in pkg.__all__ else None
    if not (isinstance(cls, type) and issubclass(cls, nn.Module)) or cls is BYOLwrapper:
        raise ValueError(f'BYOLwrapper: model_type {model_type!r} is not a model of this package')
    return cls
