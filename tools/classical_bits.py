"""The bits of the classical baselines, for comparing two builds of the library: every public function of lgteun_amd/classical.py, mtf_glp.py, bdsd.py,
cs.py, atrous.py and mtf_hr.py on tests/classical_ref.make_batch inputs (B make_scene scenes stacked, seeds 7000 + b), at the shapes the GPU tests use, and the SHA-256 of each output and of each stats tensor.
One more shape for the component-substitution modes only: (C, h, w, B) = (4, 368, 368, 1) has 529 Gram tiles against the 512 workgroups of k_cs_gram, the
smallest square shape at which one of them walks a second tile ((4, 136, 256, 1), in every list, is that shape for the moments and BDSD Gram passes).
Prints one JSON line {name: digest}.  Run it once per library and compare the lines:
    LGTEUN_HIP_LIB=/path/to/other/_lgteun_hip.so python tools/classical_bits.py > a.json;  python tools/classical_bits.py > b.json"""
import hashlib
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'tests'))
import torch  # noqa: E402

import atrous_ref as ar  # noqa: E402
import bdsd_ref as br  # noqa: E402
import classical_ref as cr  # noqa: E402
import cs_ref as csr  # noqa: E402
import mtf_glp_ref as mr  # noqa: E402
import wavelet_ref as wr  # noqa: E402
import mtf_hr_ref as hr  # noqa: E402
from lgteun_amd import atrous, bdsd, classical, cs, mtf_glp, mtf_hr  # noqa: E402

CS_SECOND_TILE = (4, 368, 368, 1)
SEED = 7


def main():
    res, batches = {}, {}

    def batch(C, h, w, B):
        if (C, h, w, B) not in batches:
            ms, pan = cr.make_batch(B, C, h, w, SEED)
            batches[C, h, w, B] = torch.from_numpy(ms).cuda(), torch.from_numpy(pan).cuda()
        return batches[C, h, w, B]

    def put(name, shape, got):
        """got: a tensor, or (output, stats)"""
        for part, t in zip(('out', 'stats'), got if isinstance(got, tuple) else (got,)):
            torch.cuda.synchronize()
            res[f'{name}.{part}@' + 'x'.join(str(v) for v in shape)] = hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    for shape in wr.SHAPES:
        ms, pan = batch(*shape)
        put('interp23', shape, classical.interp23(ms))
        put('sfim', shape, classical.sfim(ms, pan))
        put('gsa', shape, classical.gsa(ms, pan, return_stats=True))
        put('wavelet', shape, classical.wavelet(ms, pan))
    for shapes, per_band in ((mr.SHAPES, False), (mr.PER_BAND_SHAPES, True)):
        for shape in shapes:
            ms, pan = batch(*shape)
            gains = mr.per_band_gains(shape[0]) if per_band else mr.EQUAL_GAIN
            for mode in mr.MODES:
                put(f'mtf_glp_{mode}' + ('_per_band' if per_band else ''), shape, mtf_glp.mtf_glp(ms, pan, mode, gains_ms=gains, return_stats=True))
    for cases, per_band in ((br.CASES, False), (br.PER_BAND_CASES, True)):
        for *shape, block in cases:
            ms, pan = batch(*shape)
            gains = mr.per_band_gains(shape[0]) if per_band else br.EQUAL_GAIN
            put(f'bdsd_{block or "global"}' + ('_per_band' if per_band else ''), shape,
                bdsd.bdsd(ms, pan, block, gains_ms=gains, gain_pan=br.GAIN_PAN, return_stats=True))
    for shape in csr.SHAPES + [CS_SECOND_TILE]:
        ms, pan = batch(*shape)
        for mode in csr.MODES:
            put(f'cs_{mode}', shape, getattr(cs, mode)(ms, pan, return_stats=True))
    for match in ar.MATCHES:
        for shape in ar.SHAPES[match] + (ar.STATS_ONLY_SHAPES if match == 'lowpass' else []):
            ms, pan = batch(*shape)
            for rule in ar.RULES:
                put(f'{rule}_{match}', shape, atrous.atrous(ms, pan, rule, match, return_stats=True))
    for rule in hr.RULES:
        for shape in hr.SHAPES[rule] + hr.PROPERTY_SHAPES[:1]:
            ms, pan = batch(*shape)
            put(f'mtf_hr_{rule}', shape, mtf_hr.fuse(ms, pan, rule, return_stats=True))
        for shape in hr.PER_BAND_SHAPES[rule]:
            ms, pan = batch(*shape)
            put(f'mtf_hr_{rule}_per_band', shape, mtf_hr.fuse(ms, pan, rule, gains_ms=mr.per_band_gains(shape[0]), return_stats=True))
    print(json.dumps({'tool': 'classical_bits', 'lib': os.environ.get('LGTEUN_HIP_LIB', 'in-tree'), 'n': len(res), 'sha256': res}))


if __name__ == '__main__':
    main()
