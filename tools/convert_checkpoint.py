"""Convert a reference-era checkpoint to a plain state_dict file.

The reference saves whole pickled module objects: `torch.save({'core_module': <models.unlg_former.Pansharpening>,
'iter_num': n})` (models/base/base_model.py:354-369), so its checkpoints name the reference's classes.  This tool does not need
them: every class the unpickler cannot import is replaced by an empty torch.nn.Module subclass of the same name, which takes the
pickled module state (parameters, buffers, submodules) as it is, so its state_dict() lists the names and tensors the reference's
module would.  The output is a reference-free file: {'core_module': OrderedDict(name -> tensor), 'iter_num': n} that
`lgteun_amd` loads anywhere:  runner.load_checkpoint(path)  /  module.load_state_dict(ckpt['core_module']).

    python tools/convert_checkpoint.py model_iter_255000.pth model_iter_255000.state.pth
"""
import pickle
import sys
import types

import torch

_STAND_INS = {}


def _stand_in(module, name):
    """an empty nn.Module class named like the missing one: unpickling fills its __dict__ (nn.Module.__setstate__)"""
    if (module, name) not in _STAND_INS:
        _STAND_INS[module, name] = type(name, (torch.nn.Module,), {'__module__': module})
    return _STAND_INS[module, name]


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        try:
            return super().find_class(module, name)
        except (ImportError, AttributeError):
            return _stand_in(module, name)


_PICKLE = types.SimpleNamespace(__name__='convert_checkpoint_pickle', Unpickler=_Unpickler, load=lambda f, **kw: _Unpickler(f, **kw).load())


def convert(src, dst):
    ckpt = torch.load(src, map_location='cpu', weights_only=False, pickle_module=_PICKLE)
    out = {}
    for k, v in ckpt.items():
        if hasattr(v, 'state_dict'):
            v = v.module if hasattr(v, 'module') else v          # nn.DataParallel wrapper (base_model.py:363-366)
            out[k] = {n: t.detach().clone() for n, t in v.state_dict().items()}
        else:
            out[k] = v
    torch.save(out, dst)
    return out


if __name__ == '__main__':
    if len(sys.argv) != 3:
        print(__doc__)
        sys.exit(2)
    o = convert(sys.argv[1], sys.argv[2])
    print({k: (len(v) if isinstance(v, dict) else v) for k, v in o.items()})
