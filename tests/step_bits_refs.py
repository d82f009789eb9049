"""TEST INFRASTRUCTURE: the case list and the fixture of the sampler step's recorded bits (tests/golden/step_bits.npz),
shared by tools/record_step_bits.py (which writes it), tests/test_step_bits_cpu.py (the kernel on the CPU emulation) and
tests/test_step_bits_gpu.py (the kernel on the card).  The fixture holds, per case, every input of the launch and the
three outputs the library produced when it was recorded, as raw bytes: nothing is regenerated from a seed at test time.
numpy only; torch is the caller's (run_ops takes the module).
"""
import json
import os

import numpy as np

import inpaint_refs as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_bits.npz")

# ((B, C, h, w), offset): the 16-byte path on two samples; w % 4 != 0, quads that straddle rows and channels; 45 elements
# per sample (a partial last quad, sample 1 off the quads of the flat index); and the first shape with x starting `offset`
# floats behind a 16-byte boundary, which must take the scalar path at w = 8
SHAPES = [((2, 4, 8, 8), 0), ((1, 4, 3, 5), 0), ((2, 3, 3, 5), 0), ((2, 4, 8, 8), 1)]
SINGLES_ON = [SHAPES[0], SHAPES[2]]

ENTRY_POINTS = ('ddim', 'ddim_rng', 'ddim_ps', 'dpmpp', 'masked')
SIGMA = 0.3
NOISE_MUL = 0.75

_DEFAULTS = dict(solver='ddim', noise_source='none', sigma_nz=False, hist=False, ks_nz=False, nb=2, rep=1, ps=False, Bm=1)


def _forms():
    """entry point x noise source x sigma x history x ks, in full"""
    f = [dict(entry='ddim'), dict(entry='ddim', noise_source='tensor', sigma_nz=True)]
    f += [dict(entry='ddim_rng', noise_source='key', sigma_nz=s) for s in (False, True)]
    f += [dict(entry='ddim_ps', ps=True), dict(entry='ddim_ps', ps=True, noise_source='tensor', sigma_nz=True)]
    f += [dict(entry='ddim_ps', ps=True, noise_source='key', sigma_nz=s) for s in (False, True)]
    f += [dict(entry='dpmpp', solver='dpmpp', hist=h) for h in (False, True)]
    for ks in (False, True):
        f += [dict(entry='masked', noise_source='key', sigma_nz=s, ks_nz=ks) for s in (False, True)]
        f += [dict(entry='masked', noise_source='key', solver='dpmpp', hist=h, ks_nz=ks) for h in (False, True)]
    return f


def _singles():
    """nb = 1, rep = 2, a per-sample scale vector and Bm = B: once per entry point, on its fullest form"""
    full = [dict(entry='ddim', noise_source='tensor', sigma_nz=True), dict(entry='ddim_rng', noise_source='key', sigma_nz=True),
            dict(entry='ddim_ps', ps=True, noise_source='key', sigma_nz=True), dict(entry='dpmpp', solver='dpmpp', hist=True),
            dict(entry='masked', noise_source='key', sigma_nz=True, ks_nz=True),
            dict(entry='masked', noise_source='key', solver='dpmpp', hist=True, ks_nz=True)]
    out = []
    for f in full:
        out += [dict(f, nb=1), dict(f, rep=2)]
        if f['entry'] in ('dpmpp', 'masked'):
            out.append(dict(f, ps=True))
        if f['entry'] == 'masked':
            out.append(dict(f, Bm='B'))
    return out


def settings():
    """the fixed case list: one dict of settings per case (no arrays)"""
    out = []
    for forms, shapes in ((_forms(), SHAPES), (_singles(), SINGLES_ON)):
        for shape, offset in shapes:
            for f in forms:
                c = dict(_DEFAULTS, **f, shape=list(shape), offset=offset)
                if c['Bm'] == 'B':
                    c['Bm'] = shape[0]
                # the keyed cases depend on the device's logf / sinpif / cospif; the others on correctly rounded IEEE
                # operations and f16 conversion alone
                c['generator_free'] = c['noise_source'] != 'key' or not (c['sigma_nz'] or c['ks_nz'])
                c['name'] = name(c)
                out.append(c)
    assert len({c['name'] for c in out}) == len(out)
    return out


def name(c):
    s = f"{c['entry']}-{c['solver']}-{'x'.join(map(str, c['shape']))}+{c['offset']}-noise_{c['noise_source']}"
    s += f"-sigma{int(c['sigma_nz'])}-hist{int(c['hist'])}-ks{int(c['ks_nz'])}-nb{c['nb']}-rep{c['rep']}-ps{int(c['ps'])}-Bm{c['Bm']}"
    return s


INPUTS = ('eps', 'x', 'noise', 'x0_prev', 'x0_keep', 'mask', 'coef', 'scale', 'keys')
OUTPUTS = (('x_out', np.uint32), ('pred_x0', np.uint32), ('xin_next', np.uint16))


def make_inputs(c):
    """the inputs of a case, as recorded once (tools/record_step_bits.py): arrays where the launch takes one, None elsewhere;
    plus the numbers step, noise_mul, ksq, ks"""
    from lib import inpaint, solver
    shape = tuple(c['shape'])
    B, C, h, w = shape
    g = np.random.default_rng(B * 1000 + C * 100 + h * 10 + w)
    eps = g.standard_normal((2 * B, h, w, C)).astype(np.float16)
    x = g.standard_normal(shape).astype(np.float32)
    noise = g.standard_normal(shape).astype(np.float32)
    hist = (1.5 * g.standard_normal(shape)).astype(np.float32)
    x0 = (2.0 * g.standard_normal(shape)).astype(np.float32)
    index = 1 if c['ks_nz'] or c['entry'] != 'masked' else 0       # ks == 0 is the last step's constant
    scale = np.linspace(1.5, 3.0, B).astype(np.float32)
    if c['solver'] == 'ddim':
        a, ap = R.ALPHAS[index], R.ALPHAS_PREV[index]
        coef = np.array([a, ap, SIGMA if c['sigma_nz'] else 0.0, np.sqrt(1.0 - a), R.SCALE], dtype=np.float32)
    else:
        coef = solver.dpmpp_2m_table(R.ALPHAS, R.ALPHAS_PREV, R.SCALE, 2)[index].astype(np.float32)
    masked = c['entry'] == 'masked'
    ksq, ks = inpaint.step_constants(R.ALPHAS_PREV[index], index) if masked else (1.0, 0.0)
    return dict(eps=eps[:c['nb'] * B].copy(), x=x, noise=noise if c['noise_source'] == 'tensor' else None,
                x0_prev=hist if c['hist'] else None, x0_keep=x0 if masked else None,
                mask=R.mask('soft', shape, c['Bm']) if masked else None, coef=coef, scale=scale if c['ps'] else None,
                keys=R.keys(B) if c['noise_source'] == 'key' else None, step=index,
                noise_mul=NOISE_MUL if c['noise_source'] == 'key' and c['sigma_nz'] else 1.0, ksq=float(ksq), ks=float(ks))


def save(path, cases, hip_version):
    """cases: settings + inputs + the three outputs.  One byte blob (equal arrays stored once) and a JSON index."""
    blob, where, meta = bytearray(), {}, []
    for c in cases:
        m = {k: v for k, v in c.items() if not isinstance(v, np.ndarray) and v is not None}
        m['arrays'] = {}
        for k, v in c.items():
            if isinstance(v, np.ndarray):
                raw = np.ascontiguousarray(v).tobytes()
                if raw not in where:
                    where[raw] = len(blob)
                    blob += raw
                m['arrays'][k] = [where[raw], str(v.dtype), list(v.shape)]
        meta.append(m)
    index = json.dumps(dict(hip=hip_version, cases=meta)).encode()
    np.savez_compressed(path, index=np.frombuffer(index, dtype=np.uint8), blob=np.frombuffer(bytes(blob), dtype=np.uint8))


def load(path=FIXTURE):
    """-> (torch.version.hip of the recording, the cases)"""
    with np.load(path) as f:
        index, blob = json.loads(f['index'].tobytes().decode()), f['blob'].tobytes()
    cases = []
    for m in index['cases']:
        c = {k: v for k, v in m.items() if k != 'arrays'}
        for k in INPUTS + tuple(n for n, _ in OUTPUTS):
            c[k] = None
        for k, (at, dtype, shape) in m['arrays'].items():
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            c[k] = np.frombuffer(blob[at:at + n], dtype=dtype).reshape(shape)
        cases.append(c)
    return index['hip'], cases


def run_ops(c, ops, torch, device='cuda'):
    """a case through the lib.hip.ops wrapper of its entry point -> (x_out uint32, pred_x0 uint32, xin_next uint16)"""
    def dev(a):
        return None if a is None else torch.from_numpy(np.array(a)).to(device)
    n = int(np.prod(c['shape']))
    buf = torch.empty(n + c['offset'], dtype=torch.float32, device=device)     # offset: a contiguous view of a longer buffer
    x = buf[c['offset']:].view(*c['shape'])
    x.copy_(dev(c['x']))
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 * c['offset']
    eps, coef, scale, keys = dev(c['eps']), dev(c['coef']), dev(c['scale']), dev(c['keys'])
    if c['entry'] == 'masked':
        out = ops.cfg_step_masked(eps, c['nb'], x, coef, solver=c['solver'], x0_prev=dev(c['x0_prev']), keep_key=keys,
                                  step=c['step'], x0_keep=dev(c['x0_keep']), mask=dev(c['mask']), ksq=c['ksq'], ks=c['ks'],
                                  noise_mul=c['noise_mul'], scale=scale, want_next=True, rep=c['rep'])
    elif c['entry'] == 'dpmpp':
        out = ops.cfg_dpmpp_step(eps, c['nb'], x, coef, x0_prev=dev(c['x0_prev']), want_next=True, rep=c['rep'], scale=scale)
    else:
        out = ops.cfg_ddim_step(eps, c['nb'], x, coef, noise=dev(c['noise']), want_next=True, rep=c['rep'], noise_key=keys,
                                step=c['step'] if keys is not None else None, noise_mul=c['noise_mul'], scale=scale)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy().view(dt) for o, (_, dt) in zip(out, OUTPUTS))


EMU_ENTRY = {'ddim': 'ddim', 'ddim_rng': 'rng', 'ddim_ps': 'ps', 'dpmpp': 'dpmpp', 'masked': 'masked'}


def emu_case(c, path):
    """write the input file of tools/cpu_emu/emu_step.cpp for a case -> the case argument.  In the emulation every fp32
    tensor starts `offset` floats behind a 16-byte boundary."""
    coef = np.zeros(8, dtype=np.float32)
    coef[:c['coef'].size] = c['coef']
    parts = [c['keys'], coef, c['scale'], c['eps'], c['x'], c['noise'], c['x0_prev'], c['x0_keep'], c['mask']]
    with open(path, "wb") as f:
        f.write(b"".join(np.ascontiguousarray(p).tobytes() for p in parts if p is not None))
    B, C, h, w = c['shape']
    return (f"{EMU_ENTRY[c['entry']]},{B},{c['Bm']},{C},{h},{w},{c['nb']},{c['rep']},{0 if c['solver'] == 'ddim' else 1},"
            f"{int(c['scale'] is not None)},{int(c['x0_prev'] is not None)},{int(c['noise'] is not None)},"
            f"{int(c['keys'] is not None)},{c['step']},{float(c['noise_mul']).hex()},{float(c['ksq']).hex()},"
            f"{float(c['ks']).hex()},{c['offset']},{path}")


def kernel_of(c):
    """the instantiation a case must run: cfg_step_kernel<solver, keyed, masked, 16-byte access>; the 16-byte form only for
    w % 4 == 0 on aligned tensors"""
    tf = ('false', 'true')
    vec = c['shape'][3] % 4 == 0 and c['offset'] == 0
    return (f"cfg_step_kernel<{0 if c['solver'] == 'ddim' else 1}, {tf[c['keys'] is not None]}, "
            f"{tf[c['entry'] == 'masked']}, {tf[vec]}>")


def specification(c):
    """(x_out, pred_x0) of the host specification on a case: lib/inpaint.py's masked step, which is lib/solver.py's and
    lib/noise.py's un-masked step under a mask of ones"""
    from lib import inpaint
    B, C, h, w = c['shape']
    masked = c['entry'] == 'masked'
    keys = c['keys'] if c['keys'] is not None else np.zeros((B, 2), dtype=np.int64)
    assert masked or c['keys'] is not None or c['coef'][2] == 0.0 or c['solver'] != 'ddim'     # (a noise tensor has no seeded twin)
    return inpaint.masked_step(c['eps'], c['nb'], c['x'], c['coef'], keys, c['step'],
                               c['x0_keep'] if masked else np.zeros(c['shape'], dtype=np.float32),
                               c['mask'] if masked else np.ones((1, h, w), dtype=np.float32), c['ksq'], c['ks'],
                               solver=c['solver'], x0_prev=c['x0_prev'], noise_mul=c['noise_mul'], scale=c['scale'])[:2]
