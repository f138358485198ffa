"""Shared by tests/test_emu_comodgan_layers.py and tests/test_gpu_comodgan_layers.py: every Co-Mod-GAN layer checked in isolation.

One debug-plan forward keeps every layer's output (comodgan_set_debug).  Each reference-level layer is then recomputed by the
oracle in float64 FROM THE TENSOR THE DEVICE FED IT (the device's own tap, not the oracle's chained one), so no upstream error
enters a comparison and a failing unit names the faulty launch.  Styles come from the device's `mapping` and `encoder.b4.fc`
taps, which puts the affine, style and demodulation launches inside every modulated layer's unit.

Three arithmetic classes:
  f32   two-plane convolutions, fp32 storage: want = the float64 layer; ruler = the float32 torch layer on the same input
  f16   single-plane convolutions (comodgan_set_fp16_blocks): want = the factored form of oracle/comodgan_oracle.py with both
        operands rounded once to fp16 and everything else float64; ruler = float32 accumulation of the identical rounded operands
  with fp16 storage on, want is additionally rounded where the tap is stored as fp16, and one fp16 step is granted to the
        elements whose value, within the class bound, can reach a rounding tie

The bound of a class in a case is MARGIN x the largest ruler of that class in the case, relative to max(1, |want|max) of each
unit.  MARGIN = 8: a two-plane product carries about 22 significant bits against float32's 24 (x 4), summation order (x 2).
Measured rulers and errors: profiles/comodgan_layers.md.

Roundings the oracle cannot reproduce bit for bit.  Where the value that is rounded to fp16 comes out of fp32 arithmetic the
oracle does in float64 (the style scale of a modulated layer, the FIR in front of a strided convolution, the raw transposed
convolution stored as fp16), the device may legitimately round an element the other way when the value lies within its
arithmetic's error of a tie.  Those elements are found from the oracle's own pre-rounding values, and each grants the outputs
it feeds one fp16 step times |weight| (`slack`, elementwise, zero almost everywhere).  An operand that is formed exactly (the
plain layers: a power-of-two scale) has none.  Test infrastructure only."""
import importlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import comodgan_oracle as orc

pkg = importlib.import_module("mi-gan_amd")
cs = importlib.import_module("mi-gan_amd.comodgan_schema")
hb = pkg.hipbind

MARGIN = 8.0
F64, F32, H16 = torch.float64, torch.float32, torch.float16
# the `.fir` / `.raw` taps all alias the one shared tmp buffer: after a forward it holds its last writer's data,
# synthesis.b{R}.conv0.raw, which is checked as two units of its own; the others cannot be read back
SURVIVING_RAW = "synthesis.b{R}.conv0.raw"


def config(r, ch_base, ch_max):
    return cs.Config(resolution=r, ch_base=ch_base, ch_max=ch_max, num_ws=cs.default_num_ws(r))


def resolutions(cfg):
    return [2 ** k for k in range(3, cfg.resolution.bit_length())]


def excluded(cfg):
    """debug tensors that are registered but hold another launch's data after the forward (the shared tmp buffer)"""
    rs = resolutions(cfg)
    return [f"encoder.b{r}.conv1.fir" for r in rs] + [f"synthesis.b{r}.conv0.raw" for r in rs[:-1]]


def expected_units(cfg):
    """mapping, fromrgb, encoder.b4.{conv,fc}; synthesis.b4.{fc,conv,img}; 2 per encoder block; 3 per synthesis block; 2 raw units"""
    nb = len(resolutions(cfg))
    return 4 + 3 + 2 * nb + 3 * nb + 2


def noise_floats(cfg):
    return 16 + sum(2 * r * r for r in resolutions(cfg))


# ---- memory: the emulator runs on host arrays, the GPU on torch tensors -----------------------------------------------------
class HostMem:
    stream = 0

    def put(self, a):
        a = np.ascontiguousarray(a)
        buf = np.zeros(a.nbytes + 256, dtype=np.uint8)
        off = (256 - buf.ctypes.data % 256) % 256
        out = buf[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        out[...] = a
        return out

    def zeros(self, nbytes):
        return self.put(np.zeros(nbytes, dtype=np.uint8))

    def ptr(self, t):
        return t.ctypes.data

    def get(self, t):
        return np.array(t)

    def sync(self):
        pass


class TorchMem:
    def __init__(self, dev):
        self.dev = dev

    @property
    def stream(self):
        return int(torch.cuda.current_stream(self.dev).cuda_stream)

    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def zeros(self, nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)

    def ptr(self, t):
        return t.data_ptr()

    def get(self, t):
        return t.cpu().numpy()

    def sync(self):
        torch.cuda.synchronize(self.dev)


# ---- fp16 rounding with the elements a device may round the other way ------------------------------------------------------
def ulp16(v):
    """spacing of fp16 at |v| (float64 tensor)"""
    mag = v.abs().to(F64).clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(mag)) - 10)


def round16(pre, dv):
    """pre: the value that is rounded, as the oracle has it; dv: how far the device's value may be from it (float64, elementwise).
    -> (rounded, slack): slack is one fp16 step where `pre` lies within dv of a tie (the midpoints to both fp16 neighbours, which
    are unequally far at a power of two), else zero"""
    r16 = pre.to(F32).to(H16).numpy()
    r = torch.from_numpy(r16.astype(np.float64))
    up = torch.from_numpy(np.nextafter(r16, np.float16(np.inf)).astype(np.float64))
    dn = torch.from_numpy(np.nextafter(r16, np.float16(-np.inf)).astype(np.float64))
    p64 = pre.to(F64)
    dist = torch.minimum(((r + up) / 2 - p64).abs(), ((r + dn) / 2 - p64).abs())
    step = torch.maximum(up - r, r - dn)
    return r, torch.where(dist < dv, step, torch.zeros_like(step))


def act_slack(s):
    return s * float(np.sqrt(2))          # lrelu_agc is sqrt(2)-Lipschitz


def u8_of(v):
    """unit_to_u8: (y * 0.5 + 0.5).clamp(0, 1) * 255, truncated"""
    return np.floor(np.clip(v * 0.5 + 0.5, 0.0, 1.0) * 255.0)


class Layers:
    """The units of one case: the device's taps in, the oracle's layer functions on them."""

    def __init__(self, cfg, sd, taps, half, *, n, samples, psi, cutoff, noise_mode, noise, flags, x_in):
        self.cfg, self.taps, self.half = cfg, taps, half
        self.n, self.s, self.b = n, samples, n * samples
        self.psi, self.cutoff, self.noise_mode, self.flags = psi, cutoff, noise_mode, flags
        self.sd = {dt: {k: torch.from_numpy(np.asarray(v)).to(dt) for k, v in sd.items()} for dt in (F64, F32)}
        self.x_in = x_in                                    # [N,4,R,R] float64 numpy: the network input as the first layer reads it
        self.drawn = None
        if noise_mode == "random":
            self.drawn, off = {}, 0
            for nm in ["synthesis.b4.conv"] + [f"synthesis.b{r}.conv{i}" for r in resolutions(cfg) for i in (0, 1)]:
                r = 4 if nm == "synthesis.b4.conv" else int(nm.split(".")[1][1:])
                self.drawn[nm] = torch.from_numpy(noise[off:off + self.b * r * r].reshape(self.b, 1, r, r).astype(np.float64))
                off += self.b * r * r

    # -- inputs
    def tap(self, name, dt):
        t = torch.from_numpy(self.taps[name]).to(dt)
        if t.ndim == 4 and not (name.endswith(".img") or name == "y"):
            t = t.permute(0, 3, 1, 2).contiguous()          # NHWC -> NCHW
        return t

    def enc_marked(self, r):
        return r > 4 and self.flags[0] is not None and r > self.flags[0]

    def syn_marked(self, r):
        return r > 4 and self.flags[1] is not None and r > self.flags[1]

    def per_sample(self, t):
        return t if self.s == 1 else t.repeat_interleave(self.s, dim=0)

    def wlong(self, widx, dt):
        sd = self.sd[dt]
        w = self.tap("mapping", dt)
        if self.psi != 1.0 and self.cutoff is not None and widx >= self.cutoff:
            # rows past the cutoff read the un-truncated w, which is no debug tensor: the truncation of the tap undone
            w = sd["mapping.w_avg"] + (w - sd["mapping.w_avg"]) / self.psi
        return torch.cat([w, self.per_sample(self.tap("encoder.b4.fc", dt))], 1)

    def styles(self, p, widx, dt):
        sd = self.sd[dt]
        return orc.dense(self.wlong(widx, dt), sd[p + ".affine.weight"], sd[p + ".affine.bias"])

    def noise_of(self, p, dt, omit):
        if omit == "noise" or self.noise_mode == "none":
            return None
        sd = self.sd[dt]
        src = sd[p + ".noise_const"] if self.noise_mode == "const" else self.drawn[p].to(dt)
        return src * sd[p + ".noise_strength"]

    # -- layers.  Each returns (value, slack); slack is None where every rounding is reproduced exactly
    def plain_conv(self, x, p, dt, od, down=1):
        sd = self.sd[dt]
        if od is None:
            return orc.conv2d_layer(x, sd, p, down=down), None
        slack = None
        if down == 2:
            # the FIR in front: in float64 in both passes, so that the ruler's operands are want's operands
            f = orc.fir(F64)
            xin, x = x.to(F64), orc.upfirdn_pad(x.to(F64), f, (2, 2, 2, 2))
            if dt == F64:
                # the device's FIR is fp32: at most 7 roundings of 2^-24 along any path (two sums and a product per row, a product
                # and three sums down the rows), each on terms bounded by the FIR of |x|
                _, sx = round16(x, orc.upfirdn_pad(xin.abs(), f, (2, 2, 2, 2)) * 2.0 ** -21)
                w = sd[p + ".weight"].abs() * (1.0 + 2.0 ** -10)          # |w| rounded to fp16 is at most this
                slack = F.conv2d(sx, w, stride=2) * (1.0 / np.sqrt(w.shape[1] * 9))
        y = orc.conv2d_factored(x, sd[p + ".weight"], down=down, operand_dtype=od, dtype=dt) + sd[p + ".bias"].view(1, -1, 1, 1)
        return orc.act(y), None if slack is None else act_slack(slack)

    def mod_conv(self, x, p, widx, dt, od, up, raw_half=False):
        """the modulated convolution without noise, bias and activation; up=2: the raw transposed convolution (before the FIR)"""
        sd = self.sd[dt]
        if od is None:
            return orc.modulated_conv2d_factored(x, sd[p + ".weight"], self.styles(p, widx, dt), up=up, dtype=dt), None
        if raw_half and dt != F64:
            # the ruler of a unit with a rounding inside: that rounding is want's
            return self.mod_conv(x.to(F64), p, widx, F64, od, up, True)[0].to(dt), None
        st = self.styles(p, widx, F64)                       # in both passes: the ruler's operands are want's operands
        y = orc.modulated_conv2d_factored(x, sd[p + ".weight"], st, up=up, operand_dtype=od, dtype=dt)
        if dt != F64:
            return y, None
        # Which activation operands may round the other way.  The device's style scale comes out of fp32 launches (affine: a dense
        # layer over 1536 inputs; the normalisation: a reduction and three products).  How far an fp32 dense layer lands from the
        # float64 one is measured here with the float32 oracle, x 2 for the order of summation; the products add 2^-21 relative.
        dst = 2.0 * float((self.styles(p, widx, F32).to(F64) - st).abs().max())
        sa, sw, coef = orc.modulated_factors(sd[p + ".weight"], st, od)
        g = float(st.square().mean().rsqrt())
        e2 = (sa.abs().amax(dim=1) / (st * g).abs().amax(dim=1)).round().view(-1, 1)  # the power of two in sa
        dsa = (g * e2 * dst + sa.abs() * 2.0 ** -21).view(sa.shape[0], -1, 1, 1)
        pre = x.to(F32) * sa.to(F32).view(sa.shape[0], -1, 1, 1)
        _, sx = round16(pre, x.abs() * dsa + pre.abs().to(F64) * 2.0 ** -23)
        w16 = (sd[p + ".weight"].to(F32) * sw.to(F32)).to(H16).to(F64).abs()
        slack = torch.cat([orc.conv_taps(sx[i:i + 1], w16, up) * coef[i].view(1, -1, 1, 1) for i in range(x.shape[0])], 0)
        if raw_half:
            # the stored raw tensor: rounded the other way where the class's accumulation bound and the flips above reach a tie
            y32 = orc.modulated_conv2d_factored(x.to(F32), self.sd[F32][p + ".weight"], st, up=up, operand_dtype=od, dtype=F32).to(F64)
            y, s2 = round16(y, MARGIN * float((y32 - y).abs().max()) + slack)
            slack = slack + s2
        return y, slack

    def mod_layer(self, x, p, widx, dt, od, omit, up=1, raw_half=False):
        sd = self.sd[dt]
        if od is None and not raw_half:
            mode = "none" if omit == "noise" else self.noise_mode
            return orc.synthesis_layer(x, self.wlong(widx, dt), sd, p, up=up, noise_mode=mode,
                                       drawn=None if self.drawn is None else {k: v.to(dt) for k, v in self.drawn.items()}), None
        y, slack = self.mod_conv(x, p, widx, dt, od, up, raw_half)
        return self.finish(y, slack, p, dt, omit, up)

    def finish(self, y, slack, p, dt, omit, up):
        """behind the contraction: FIR of the up path, noise, bias, activation"""
        sd = self.sd[dt]
        if up == 2:
            f = orc.fir(dt)
            y = orc.upfirdn_pad(y, f, (1, 1, 1, 1), gain=4.0)
            if slack is not None:
                slack = orc.upfirdn_pad(slack, orc.fir(F64), (1, 1, 1, 1), gain=4.0)
        nz = self.noise_of(p, dt, omit)
        if nz is not None:
            y = y + nz
        return orc.act(y + sd[p + ".bias"].view(1, -1, 1, 1)), None if slack is None else act_slack(slack)

    def od(self, marked):
        return H16 if marked else None

    def units(self):
        """-> [(name, tap, cls, fn(dt, omit) -> (value, slack), omittable terms)] in launch order"""
        cfg, R, S = self.cfg, self.cfg.resolution, self.s
        rs = resolutions(cfg)
        n_layers = sum(1 for k in self.sd[F64] if k.startswith("mapping.fc") and k.endswith(".weight"))
        u = []

        def add(name, tap, cls, fn, terms=()):
            u.append((name, tap, cls, fn, tuple(t for t in terms if not (t == "noise" and self.noise_mode == "none"))))

        z = self.z
        add("mapping", "mapping", "f32", lambda dt, o: (orc.mapping(torch.from_numpy(z).to(dt), self.sd[dt], cfg.num_ws, n_layers, self.psi,
                                                                    self.cutoff)[:, 0], None))
        add(f"encoder.b{R}.fromrgb", f"encoder.b{R}.fromrgb", "f32",
            lambda dt, o: (orc.conv2d_layer(torch.from_numpy(self.x_in).to(dt), self.sd[dt], f"encoder.b{R}.fromrgb", k=1), None))
        prev = f"encoder.b{R}.fromrgb"
        for r in reversed(rs):
            p, od = f"encoder.b{r}", self.od(self.enc_marked(r))
            cls = "f16" if od is not None else "f32"

            def conv0(dt, o, p=p, od=od, prev=prev):
                return self.plain_conv(self.tap(prev, dt), p + ".conv0", dt, od)

            def conv1(dt, o, p=p, od=od):
                return self.plain_conv(self.tap(p + ".conv0", dt), p + ".conv1", dt, od, down=2)

            add(p + ".conv0", p + ".conv0", cls, conv0)
            add(p + ".conv1", p + ".conv1", cls, conv1)
            prev = p + ".conv1"
        add("encoder.b4.conv", "encoder.b4.conv", "f32", lambda dt, o, prev=prev: self.plain_conv(self.tap(prev, dt), "encoder.b4.conv", dt, None))
        add("encoder.b4.fc", "encoder.b4.fc", "f32",
            lambda dt, o: (orc.dense(self.tap("encoder.b4.conv", dt).flatten(1), self.sd[dt]["encoder.b4.fc.weight"],
                                     self.sd[dt]["encoder.b4.fc.bias"], activation=True), None))

        def syn_fc(dt, o):
            sd = self.sd[dt]
            y = orc.dense(self.tap("encoder.b4.fc", dt), sd["synthesis.b4.fc.weight"], sd["synthesis.b4.fc.bias"], activation=True)
            y = y.view(y.shape[0], -1, 4, 4)
            if o != "skip":
                y = y + self.tap("encoder.b4.conv", dt)
            return self.per_sample(y), None

        add("synthesis.b4.fc", "synthesis.b4.fc", "f32", syn_fc, ("skip",))
        add("synthesis.b4.conv", "synthesis.b4.conv", "f32",
            lambda dt, o: self.mod_layer(self.tap("synthesis.b4.fc", dt), "synthesis.b4.conv", 0, dt, None, o), ("noise",))
        add("synthesis.b4.img", "synthesis.b4.img", "f32",
            lambda dt, o: (orc.torgb_layer(self.tap("synthesis.b4.conv", dt), self.wlong(1, dt), self.sd[dt], "synthesis.b4.torgb"), None))
        xprev, imprev, widx = "synthesis.b4.conv", "synthesis.b4.img", 1
        for r in rs:
            p, od = f"synthesis.b{r}", self.od(self.syn_marked(r))
            cls = "f16" if od is not None else "f32"
            raw_half = self.half.get(p + ".conv0.raw", False) if r == R else bool(self.half.get(p + ".conv0") and self.half.get(xprev))

            def skip_of(dt, r=r):
                return self.per_sample(self.tap(f"encoder.b{r}.conv0", dt))

            def conv0(dt, o, p=p, od=od, xprev=xprev, widx=widx, raw_half=raw_half, skip_of=skip_of):
                y, s = self.mod_layer(self.tap(xprev, dt), p + ".conv0", widx, dt, od, o, up=2, raw_half=raw_half)
                return (y if o == "skip" else y + skip_of(dt)), s

            def conv1(dt, o, p=p, od=od, widx=widx):
                return self.mod_layer(self.tap(p + ".conv0", dt), p + ".conv1", widx + 1, dt, od, o)

            def img(dt, o, p=p, widx=widx, imprev=imprev):
                y = orc.torgb_layer(self.tap(p + ".conv1", dt), self.wlong(widx + 2, dt), self.sd[dt], p + ".torgb")
                return (y if o == "prev" else y + orc.upsample2d(self.tap(imprev, dt), orc.fir(dt))), None

            add(p + ".conv0", p + ".conv0", cls, conv0, ("skip", "noise"))
            if r == R:
                def raw(dt, o, p=p, od=od, xprev=xprev, widx=widx, raw_half=raw_half):
                    return self.mod_conv(self.tap(xprev, dt), p + ".conv0", widx, dt, od, 2, raw_half)

                def from_raw(dt, o, p=p, skip_of=skip_of):
                    y, _ = self.finish(self.tap(p + ".conv0.raw", dt), None, p + ".conv0", dt, o, 2)
                    return (y if o == "skip" else y + skip_of(dt)), None

                add(p + ".conv0.raw", p + ".conv0.raw", cls, raw)
                add(p + ".conv0.raw->conv0", p + ".conv0", "f32", from_raw, ("skip", "noise"))
            add(p + ".conv1", p + ".conv1", cls, conv1, ("noise",))
            add(p + ".img", "y" if r == R else p + ".img", "f32", img, ("prev",))
            xprev, imprev, widx = p + ".conv1", p + ".img", widx + 2
        return u


def check_layers(lib, mem, cfg, sd, x, z, *, psi=1.0, cutoff=None, noise_mode="const", noise=None, flags=(None, None), storage=False,
                 samples=1, u8=None, kernels=(), tag="", report=None, premise=None):
    """One normal-plan and one debug-plan forward on a fresh handle; every assertion the layer test makes.  x [N,4,R,R] (or None
    with u8 = (img [N,R,R,3], mask [N,R,R])), z [N*S, z_dim].  premise(L): what the case claims to reach, asserted on the Layers
    object once L.wants / L.fns hold every unit's float64 value and function (never on the device's output).
    -> (rows of the per-unit table, unit count)"""
    R, S = cfg.resolution, samples
    n = (u8[0] if u8 is not None else x).shape[0]
    B = n * S
    h = hb.CoModGANHandle(lib, R, cfg.num_ws, cfg.ch_base, cfg.ch_max, cfg.z_dim, cfg.w_dim, cfg.w0_dim, cfg.map_layers)
    keep = {k: mem.put(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
    for name, shape, _ in h.weights():
        h.set_weight(name, mem.ptr(keep[name]), shape)
    h.commit(mem.stream)
    if cutoff is not None:
        h.set_truncation_cutoff(cutoff)
    h.set_fp16_blocks(*flags)
    if storage:
        h.set_fp16_storage(True)
    zd = mem.put(np.asarray(z, dtype=np.float32))
    nd = None if noise is None else mem.put(np.asarray(noise, dtype=np.float32))
    ins = [mem.put(u8[0]), mem.put(u8[1])] if u8 is not None else [mem.put(np.asarray(x, dtype=np.float32))]

    def forward(debug):
        h.set_debug(debug)
        nbytes = h.workspace_bytes_samples(n, S)
        ws = mem.zeros(nbytes)
        y = mem.zeros(B * 3 * R * R * (1 if u8 is not None else 4))
        nptr = None if nd is None else mem.ptr(nd)
        if u8 is not None:
            h.forward_u8(mem.ptr(ins[0]), mem.ptr(ins[1]), mem.ptr(zd), mem.ptr(y), n, S, mem.ptr(ws), nbytes, psi, noise_mode, nptr, mem.stream)
        elif S == 1:
            h.forward(mem.ptr(ins[0]), mem.ptr(zd), mem.ptr(y), n, mem.ptr(ws), nbytes, psi, noise_mode, nptr, mem.stream)
        else:
            h.forward_samples(mem.ptr(ins[0]), mem.ptr(zd), mem.ptr(y), n, S, mem.ptr(ws), nbytes, psi, noise_mode, nptr, mem.stream)
        mem.sync()
        info = [(i["layer"], i["kernel"]) for i in h.launches()]
        yh = mem.get(y)
        yh = yh.reshape(B, R, R, 3) if u8 is not None else yh.view(np.float32).reshape(B, 3, R, R)
        return yh, info, mem.get(ws)

    y_normal, info_normal, _ = forward(False)
    y_debug, info_debug, ws_host = forward(True)
    # the two plans run the same kernels on the same operands: only the buffers and the side stream differ
    assert info_debug == info_normal, (tag, [a for a in zip(info_debug, info_normal) if a[0] != a[1]][:4])
    # (bytes, not values: an output that is NaN in both plans goes on to the units below, which name the launch it came from)
    assert y_debug.tobytes() == y_normal.tobytes(), (tag, "y differs between the debug and the normal plan")
    kernel_of = dict(info_debug)
    if report is not None:
        report["kernels"] = sorted(set(kernel_of.values()))
    missing = set(kernels) - set(kernel_of.values())
    assert not missing, (tag, missing, sorted(set(kernel_of.values())))

    names = ["mapping", f"encoder.b{R}.fromrgb", "encoder.b4.conv", "encoder.b4.fc", "synthesis.b4.fc", "synthesis.b4.conv", "synthesis.b4.img"]
    for r in resolutions(cfg):
        names += [f"encoder.b{r}.conv0", f"encoder.b{r}.conv1", f"synthesis.b{r}.conv0", f"synthesis.b{r}.conv1"]
        names += [f"synthesis.b{r}.img"] if r != R else [SURVIVING_RAW.format(R=R)]
    taps, half = {}, {}
    for name in names:
        taps[name] = h.read_debug_tensor(ws_host, n, name, samples=S)
        half[name] = h.debug_tensor_dtype(n, name, samples=S) == hb.COMODGAN_DTYPE_F16
    for name in excluded(cfg):
        h.debug_tensor_samples(n, S, name)                  # registered, and knowingly not compared (see excluded())
    h.close()
    assert any(half.values()) == (storage and any(f is not None for f in flags)), (tag, half)
    taps["y"] = y_debug
    if u8 is None:
        x_in = np.asarray(x, dtype=np.float64)
    else:
        # migan_pack_input's formula: x = cat([mask - 0.5, (img * 2 / 255 - 1) * mask]), mask = (byte == 255)
        mk = (u8[1] == 255).astype(np.float64)[:, None]
        x_in = np.concatenate([mk - 0.5, (np.transpose(u8[0].astype(np.float64), (0, 3, 1, 2)) * 2.0 / 255.0 - 1.0) * mk], 1)
    half["y"] = False

    L = Layers(cfg, sd, taps, half, n=n, samples=S, psi=psi, cutoff=cutoff, noise_mode=noise_mode, noise=noise, flags=flags, x_in=x_in)
    L.z = np.asarray(z, dtype=np.float32)
    units = L.units()
    with torch.no_grad():
        # the class of a convolution unit is the kernel family the plan names for it
        for name, tap, cls, fn, terms in units:
            ks = [k for l, k in info_debug if (l == name or l.startswith(name + ".phase")) and "cm_conv" in k]
            if ks and not name.endswith("->conv0"):
                single = ["cm_conv_f16_kernel" in k or "cm_conv_h_kernel" in k for k in ks]
                assert all(single) == (cls == "f16") and any(single) == (cls == "f16"), (tag, name, ks)
        rows, res = [], []
        for name, tap, cls, fn, terms in units:
            want, slack = fn(F64, None)
            base32 = fn(F32, None)[0]
            ruler = base32.to(F64)
            ruler_err = float((ruler - want).abs().max())          # before any rounding of the stored value
            res.append((name, tap, cls, fn, terms, want, slack, ruler_err, base32))
        bound = {}
        for cls in ("f32", "f16"):
            rr = [ruler_err / max(1.0, float(want.abs().max())) for _, _, c, _, _, want, _, ruler_err, _ in res if c == cls]
            if rr:
                bound[cls] = MARGIN * max(rr)
        failures, vacuous = [], []
        for name, tap, cls, fn, terms, want, slack, ruler_err, base32 in res:
            wmax = float(want.abs().max())
            scale = max(1.0, wmax)
            b_abs = bound[cls] * scale
            if half[tap] and tap != "y":
                # stored as fp16: want rounded too; one fp16 step where the device's value, within the bound of want, can reach a tie
                want, s_out = round16(want, b_abs + (0 if slack is None else slack))
                slack = s_out if slack is None else slack + s_out
            if u8 is not None and tap == "y":
                # the composited bytes: a hole pixel is unit_to_u8 of a value within the bound of want, a known pixel the photo's byte
                got = taps["y"].astype(np.float64)
                w = np.transpose(want.numpy(), (0, 2, 3, 1))
                known = np.repeat((u8[1] == 255), S, axis=0)[..., None]
                photo = np.repeat(u8[0].astype(np.float64), S, axis=0)
                lo, hi = np.where(known, photo, u8_of(w - b_abs)), np.where(known, photo, u8_of(w + b_abs))
                bad = (got < lo) | (got > hi)
                err = 0.0 if not bad.any() else float("inf")
                assert (~known).mean() >= 0.2 and np.ptp(u8_of(w)[np.broadcast_to(~known, w.shape)]) > 50, (tag, "uint8 unit is vacuous")
            else:
                got = L.tap(tap, F64)
                assert got.shape == want.shape, (tag, name, got.shape, want.shape)
                diff = (got - want).abs()
                err = float((diff if slack is None else (diff - slack).clamp_min(0)).max())
            rows.append(dict(case=tag, unit=name, cls=cls + ("+st" if half[tap] and tap != "y" else ""), wmax=wmax, ruler=ruler_err / scale,
                             err=err / scale, bound=bound[cls], slack=0.0 if slack is None else float(torch.as_tensor(slack).max()) / scale))
            if not np.isfinite(err) or err > b_abs:
                failures.append((name, cls, err / scale, bound[cls], err / b_abs))
            # guards: the unit cannot pass vacuously
            if not wmax >= 100 * b_abs:
                vacuous.append((name, "|want|max below 100 x the bound", wmax, b_abs))
            for term in terms:
                d = float((fn(F32, term)[0] - base32).abs().max())
                if not d > 10 * b_abs:
                    vacuous.append((name, f"the {term} term is below 10 x the bound", d, b_abs))
        print(format_rows(rows))
        # a faulty launch first: a NaN or an unclamped value that it hands on makes the units behind it look vacuous
        assert not failures, (tag, "units over their bound (unit, class, error, bound, ratio)", failures)
        assert not vacuous, (tag, "units that could pass vacuously", vacuous)
        # after the units, so that a faulty launch is reported as such and not as the premise it breaks downstream
        if premise is not None:
            L.wants, L.fns = {r[0]: r[5] for r in res}, {r[0]: r[3] for r in res}
            notes = premise(L)
            print(tag, "premises reached:", notes)
            if report is not None:
                report["premise"] = notes
    return rows, len(units)


def format_rows(rows):
    out = ["| case | unit | class | max abs want | ruler | device error | bound | error / bound | max slack |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['case']} | {r['unit']} | {r['cls']} | {r['wmax']:.3g} | {r['ruler']:.2e} | {r['err']:.2e} | {r['bound']:.2e} | "
                   f"{r['err'] / r['bound']:.2f} | {r['slack']:.1e} |")
    return "\n".join(out)


# ---- the cases: the smallest shapes that reach every kernel form ---------------------------------------------------------------
# name -> dict(cfg=(R, ch_base, ch_max), n, seed, env, kernels, and check_layers' options)
def _case(cfg, n, seed, env=None, kernels=(), **kw):
    return dict(cfg=cfg, n=n, seed=seed, env=env or {}, kernels=tuple(kernels), kw=kw)


def K(*names):
    return tuple("migan::" + n for n in names)


R16, R32, R32W, R16W, R64 = (16, 1024, 64), (32, 4096, 128), (32, 2048, 256), (16, 8192, 256), (64, 4096, 64)
CASES = {
    # 64-column plain, strided and four-phase kernels; the noise epilogues; ToRGB on 4 lanes; an odd batch
    "r16_const": _case(R16, 3, 101,
        kernels=K("cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    "r16_none": _case(R16, 3, 102, noise_mode="none",
        kernels=K("cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    "r16_random": _case(R16, 3, 103, random_noise=True,
        kernels=K("cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    # 128-column plain, <128,16,9> strided, four-phase on 64 and on 128 columns, single-phase tap lists; truncation with a cutoff,
    # so that the affine launch reads both latent rows
    "r32": _case(R32, 2, 104, psi=0.7, cutoff=3,
        kernels=K("cm_conv_kernel<128, 16, 9, true, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<8>")),
    "r32_up4_0": _case(R32, 2, 105, env={"COMODGAN_UP4": "0"}, psi=0.7, cutoff=3,
        kernels=K("cm_conv_kernel<128, 16, 9, true, 2, false>", "cm_conv_kernel<128, 32, 6, false, 2, false>",
                  "cm_conv_kernel<128, 32, 6, true, 2, false>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<8>")),
    "r32_up4_nt128": _case(R32, 2, 106, env={"COMODGAN_UP4_NT": "128"},
        kernels=K("cm_conv_kernel<128, 16, 9, true, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, false>",
                  "cm_conv_kernel<128, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<8>")),
    # ToRGB on 16, 8 and 4 lanes per pixel; 256 channels at res 4 and 8
    "r32_c256": _case(R32W, 1, 107,
        kernels=K("cm_conv_kernel<128, 16, 9, true, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_kernel", "cm_torgb_kernel<16>", "cm_torgb_kernel<4>", "cm_torgb_kernel<8>")),
    # <256, ..., 4> plain, strided and tap-list kernels
    "r16_c256_mti4": _case(R16W, 1, 108, env={"COMODGAN_MTI": "4", "COMODGAN_UP4": "0"},
        kernels=K("cm_conv_kernel<256, 16, 18, true, 4, false>", "cm_conv_kernel<256, 32, 11, false, 4, false>",
                  "cm_conv_kernel<256, 32, 11, true, 4, false>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<16>")),
    # several tiles per image on 16 x 16 and on 8 x 16 tiles: every tile seam and image border of conv, FIR-down, FIR-up
    "r64": _case(R64, 2, 109,
        kernels=K("cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    "r64_mti2": _case(R64, 2, 110, env={"COMODGAN_MTI": "2", "COMODGAN_UP4": "1"},
        kernels=K("cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    # single-plane and typed forms on 128 columns
    "r32_f16": _case(R32, 2, 111, flags=(8, 8),
        kernels=K("cm_conv_f16_kernel<128, 16, 9, true, 2, false>", "cm_conv_f16_kernel<128, 32, 6, true, 2, false>",
                  "cm_conv_f16_kernel<64, 32, 6, true, 2, true>", "cm_conv_kernel<128, 16, 9, true, 2, false>",
                  "cm_conv_kernel<128, 32, 6, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_kernel", "cm_torgb_kernel<8>")),
    "r32_f16_st": _case(R32, 2, 112, flags=(8, 8), storage=True,
        kernels=K("cm_conv_f16_kernel<64, 32, 6, true, 2, true>", "cm_conv_h_kernel<128, 16, 9, true, 2, false, false>",
                  "cm_conv_h_kernel<128, 16, 9, true, 2, false, true>", "cm_conv_h_kernel<128, 32, 6, true, 2, false, true>",
                  "cm_conv_h_kernel<64, 32, 6, true, 2, true, true>", "cm_conv_kernel<128, 16, 9, true, 2, false>",
                  "cm_conv_kernel<128, 32, 6, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_h_kernel<0, true, true, false>",
                  "cm_fir_h_kernel<1, false, true, true>", "cm_fir_h_kernel<1, true, true, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_h_kernel", "cm_torgb_h_kernel<8>", "cm_torgb_kernel<8>")),
    "r32_f16_up4_0": _case(R32, 2, 113, env={"COMODGAN_UP4": "0"}, flags=(8, 8),
        kernels=K("cm_conv_f16_kernel<128, 16, 9, true, 2, false>", "cm_conv_f16_kernel<128, 32, 6, false, 2, false>",
                  "cm_conv_f16_kernel<128, 32, 6, true, 2, false>", "cm_conv_kernel<128, 16, 9, true, 2, false>",
                  "cm_conv_kernel<128, 32, 6, false, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, false>", "cm_fir_kernel<0>",
                  "cm_fir_kernel<1>", "cm_fromrgb_kernel", "cm_torgb_kernel<8>")),
    "r32_f16_st_up4_0": _case(R32, 2, 114, env={"COMODGAN_UP4": "0"}, flags=(8, 8), storage=True,
        kernels=K("cm_conv_f16_kernel<128, 32, 6, false, 2, false>", "cm_conv_h_kernel<128, 16, 9, true, 2, false, false>",
                  "cm_conv_h_kernel<128, 16, 9, true, 2, false, true>", "cm_conv_h_kernel<128, 32, 6, false, 2, false, true>",
                  "cm_conv_h_kernel<128, 32, 6, true, 2, false, true>", "cm_conv_kernel<128, 16, 9, true, 2, false>",
                  "cm_conv_kernel<128, 32, 6, false, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, false>",
                  "cm_fir_h_kernel<0, true, true, false>", "cm_fir_h_kernel<1, false, true, true>", "cm_fir_h_kernel<1, true, true, true>",
                  "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_h_kernel", "cm_torgb_h_kernel<8>", "cm_torgb_kernel<8>")),
    "r32_f16_nt128": _case(R32, 2, 115, env={"COMODGAN_UP4_NT": "128"}, flags=(8, 8),
        kernels=K("cm_conv_f16_kernel<128, 16, 9, true, 2, false>", "cm_conv_f16_kernel<128, 32, 6, true, 2, false>",
                  "cm_conv_f16_kernel<128, 32, 6, true, 2, true>", "cm_conv_kernel<128, 16, 9, true, 2, false>",
                  "cm_conv_kernel<128, 32, 6, true, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_kernel", "cm_torgb_kernel<8>")),
    "r32_f16_st_nt128": _case(R32, 2, 116, env={"COMODGAN_UP4_NT": "128"}, flags=(8, 8), storage=True,
        kernels=K("cm_conv_f16_kernel<128, 32, 6, true, 2, true>", "cm_conv_h_kernel<128, 16, 9, true, 2, false, false>",
                  "cm_conv_h_kernel<128, 16, 9, true, 2, false, true>", "cm_conv_h_kernel<128, 32, 6, true, 2, false, true>",
                  "cm_conv_h_kernel<128, 32, 6, true, 2, true, true>", "cm_conv_kernel<128, 16, 9, true, 2, false>",
                  "cm_conv_kernel<128, 32, 6, true, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, true>", "cm_fir_h_kernel<0, true, true, false>",
                  "cm_fir_h_kernel<1, false, true, true>", "cm_fir_h_kernel<1, true, true, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_h_kernel", "cm_torgb_h_kernel<8>", "cm_torgb_kernel<8>")),
    # ... on 64 columns; (None, 4): fp32 skip tensors into fp16 blocks
    "r64_f16": _case(R64, 2, 117, flags=(16, 16),
        kernels=K("cm_conv_f16_kernel<64, 16, 9, true, 2, false>", "cm_conv_f16_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_f16_kernel<64, 32, 6, true, 2, true>", "cm_conv_kernel<64, 16, 9, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    "r64_f16_st": _case(R64, 2, 118, flags=(16, 16), storage=True,
        kernels=K("cm_conv_f16_kernel<64, 32, 6, true, 2, true>", "cm_conv_h_kernel<64, 16, 9, true, 2, false, false>",
                  "cm_conv_h_kernel<64, 16, 9, true, 2, false, true>", "cm_conv_h_kernel<64, 32, 6, true, 2, false, true>",
                  "cm_conv_h_kernel<64, 32, 6, true, 2, true, true>", "cm_conv_kernel<64, 16, 9, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_h_kernel<0, true, true, false>",
                  "cm_fir_h_kernel<1, false, true, true>", "cm_fir_h_kernel<1, true, true, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_h_kernel", "cm_torgb_h_kernel<4>", "cm_torgb_kernel<4>")),
    "r64_f16_syn": _case(R64, 2, 119, flags=(None, 4),
        kernels=K("cm_conv_f16_kernel<64, 32, 6, true, 2, false>", "cm_conv_f16_kernel<64, 32, 6, true, 2, true>",
                  "cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>", "cm_fir_kernel<0>", "cm_fir_kernel<1>",
                  "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    "r64_f16_syn_st": _case(R64, 2, 120, flags=(None, 4), storage=True,
        kernels=K("cm_conv_f16_kernel<64, 32, 6, true, 2, true>", "cm_conv_h_kernel<64, 32, 6, true, 2, false, true>",
                  "cm_conv_h_kernel<64, 32, 6, true, 2, true, true>", "cm_conv_kernel<64, 16, 9, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, false>", "cm_fir_h_kernel<1, false, true, false>", "cm_fir_h_kernel<1, true, true, false>",
                  "cm_fir_kernel<0>", "cm_fromrgb_kernel", "cm_torgb_h_kernel<4>", "cm_torgb_kernel<4>")),
    # an fp16 skip tensor read by an fp32 synthesis block
    "r32_f16_skip_st": _case(R32, 2, 121, flags=(8, 16), storage=True,
        kernels=K("cm_conv_f16_kernel<64, 32, 6, true, 2, true>", "cm_conv_h_kernel<128, 16, 9, true, 2, false, false>",
                  "cm_conv_h_kernel<128, 16, 9, true, 2, false, true>", "cm_conv_h_kernel<128, 32, 6, true, 2, false, true>",
                  "cm_conv_kernel<128, 16, 9, true, 2, false>", "cm_conv_kernel<128, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_h_kernel<0, true, true, false>", "cm_fir_h_kernel<1, false, false, true>",
                  "cm_fir_h_kernel<1, false, true, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_h_kernel", "cm_torgb_h_kernel<8>",
                  "cm_torgb_kernel<8>")),
    # encoder units at batch 2, synthesis units at batch 6 against image b / S
    "r16_samples": _case(R16, 2, 122, samples=3,
        kernels=K("cm_bcast_kernel", "cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_dense_multi_samples_kernel", "cm_fir_kernel<0>", "cm_fir_samples_kernel",
                  "cm_fromrgb_kernel", "cm_torgb_kernel<4>")),
    # FromRGB from bytes and the composited last ToRGB
    "r16_u8": _case(R16, 2, 123, bytes=True,
        kernels=K("cm_conv_kernel<64, 16, 9, true, 2, false>", "cm_conv_kernel<64, 32, 6, true, 2, false>",
                  "cm_conv_kernel<64, 32, 6, true, 2, true>", "cm_fir_kernel<0>", "cm_fir_kernel<1>", "cm_fromrgb_u8_kernel<false>",
                  "cm_torgb_u8_kernel<4, false>")),
}

# 16 x 16 pixel tiles exist with 256 output columns only, so the 64-channel R = 64 cases above stay on 8 x 16 tiles whatever
# COMODGAN_MTI says.  Several 16 x 16 tiles per image (their seams in the plain convolution) need 256 channels at res 32: minutes
# in the emulator, so this case runs on the GPU only.
GPU_CASES = {
    "r32_c256_mti4": _case((32, 8192, 256), 1, 124, env={"COMODGAN_MTI": "4"},
                           kernels=K("cm_conv_kernel<256, 32, 11, true, 4, false>", "cm_conv_kernel<256, 16, 18, true, 4, false>")),
}


# ---- at the bounds the operand scaling is derived from -------------------------------------------------------------------------
# kCmInBound = 512 (a convolution input: 256 from lrelu_agc's clamp + 256 of skip tensor), kCmF16Top = 2^15 (the scaled A operand)
# and the per-sample style exponent e = 6 - (floor(log2 mx) + 1) of cm_style_block.  Random weights stay two orders of magnitude
# below all three, so the cases below dress the state dict until every layer sits on them.
def demodulated(cfg):
    """[(prefix, widx, input tap)] of the modulated 3x3 layers, in launch order"""
    out, prev = [("synthesis.b4.conv", 0, "synthesis.b4.fc")], "synthesis.b4.conv"
    for k, r in enumerate(resolutions(cfg)):
        out += [(f"synthesis.b{r}.conv0", 1 + 2 * k, prev), (f"synthesis.b{r}.conv1", 2 + 2 * k, f"synthesis.b{r}.conv0")]
        prev = f"synthesis.b{r}.conv1"
    return out


def pinned_m(t, ci):
    """|style| of the one channel whose normalised value is t when the other ci - 1 styles are +-1: t = m * sqrt(ci / (ci - 1 + m^2))"""
    assert 1.0 < t * t < ci
    return float(np.sqrt(np.float64(t) ** 2 * (ci - 1) / (ci - np.float64(t) ** 2)))


def dress(cfg, sd, styles=None):
    """A copy of a make_comodgan_state_dict() result that drives every layer to its bounds.
    Locked channels: in every bias in front of an lrelu_agc that produces a feature map (the conv_b entries, and synthesis.b4.fc's by
    channel), channel co % 4 == 1 becomes +1e5 and co % 4 == 3 becomes -1e5: exactly +256 / -256 behind the clamp whatever the input.
    The encoder's skip tensor and the synthesis conv0 it is added to are locked on the same channels with the same sign, so a
    synthesis conv1 (and synthesis.b4.conv) reads exactly +-512 there.  The other half of the channels stays as drawn.
    styles = t: the largest normalised style of every demodulated layer is pinned to t, on channel 1 (a +256 / +512 channel): the
    affine weight becomes zero and the affine bias +1, -1, +1, ... with channel 1 = -m (pinned_m).  t = 1.0: all +-1, so that the
    normalised styles are exactly +-1 and mx is exactly a power of two.  ToRGB affines stay."""
    out = {k: np.array(v, copy=True) for k, v in sd.items()}

    def lock(b, co):
        b[co % 4 == 1], b[co % 4 == 3] = 1e5, -1e5

    for e in cs.entries(cfg):
        if e.role == "conv_b" and not e.name.startswith("mapping."):
            lock(out[e.name], np.arange(e.shape[0]))
    lock(out["synthesis.b4.fc.bias"], np.arange(out["synthesis.b4.fc.bias"].shape[0]) // 16)
    if styles is not None:
        for p, _, _ in demodulated(cfg):
            b = out[p + ".affine.bias"]
            out[p + ".affine.weight"][...] = 0.0
            b[0::2], b[1::2] = 1.0, -1.0
            if styles != 1.0:
                b[1] = -pinned_m(styles, b.shape[0])
    return out


def below_a_power_of_two(t):
    return float(np.frexp(t)[0]) >= 0.75


def dressed_premise(styles):
    """What a dressed case claims to reach, on the oracle's float64 values and the dressed weights only.  -> the figures reached"""
    def check(L):
        cfg, sd, notes = L.cfg, L.sd[F64], {}
        weakest = min(abs(float(sd[p + ".noise_strength"])) for p, _, _ in demodulated(cfg))
        assert weakest >= MIN_NOISE_STRENGTH, ("this seed draws a noise strength the guards cannot see", weakest)
        top = {}
        for name in L.wants:
            if name in ("mapping", "encoder.b4.fc") or name.endswith((".img", ".raw")):
                continue
            skipped = name == "synthesis.b4.fc" or (name.startswith("synthesis.") and name.endswith((".conv0", "->conv0")))
            top[name] = 512.0 if skipped else 256.0
        assert len(top) == 4 + 4 * len(resolutions(cfg)) + 1, sorted(top)
        inside = {}
        for name, tv in top.items():
            w = L.wants[name]
            assert bool((w == tv).any()) and bool((w == -tv).any()) and float(w.abs().max()) == tv, (name, tv, float(w.abs().max()))
            # strictly inside the clamp: of the activation, so before the skip tensor is added where there is one
            v = w if tv == 256.0 else L.fns[name](F64, "skip")[0]
            inside[name] = float((v.abs() < 256.0).double().mean())
            assert inside[name] >= 0.25, (name, "elements strictly inside the clamp", inside[name])
        notes["least fraction inside the clamp"] = min(inside.values())
        if styles is None:
            return notes
        rel, prod = [], {}
        for p, widx, src in demodulated(cfg):
            assert not sd[p + ".affine.weight"].any()
            st = sd[p + ".affine.bias"]
            mx = float((st * st.square().mean().rsqrt()).abs().max())
            rel.append(abs(mx / styles - 1.0))
            assert rel[-1] <= 2.0 ** -15, (p, mx, styles)
            if p.endswith(".conv0"):
                continue
            sa = orc.modulated_factors(sd[p + ".weight"], L.styles(p, widx, F64))[0]
            prod[p] = float((L.tap(src, F64) * sa.view(sa.shape[0], -1, 1, 1)).abs().max())
            if below_a_power_of_two(styles):
                assert 2.0 ** 15 * (1 - 2.0 ** -12) <= prod[p] < 2.0 ** 15, (p, prod[p])
            else:
                assert 2.0 ** 14 <= prod[p] <= 2.0 ** 14 * (1 + 2.0 ** -11), (p, prod[p])
        notes["largest |mx / t - 1|"] = max(rel)
        notes["|x * sa|max / 2^15, least and largest"] = (min(prod.values()) / 2.0 ** 15, max(prod.values()) / 2.0 ** 15)
        return notes
    return check


MIN_NOISE_STRENGTH = 0.04
HUGE_PIXELS = ((0, 1, 3, 5, np.inf), (1, 2, 9, 12, -np.inf), (2, 3, 15, 0, 3e38))      # (image, plane, row, column, value)


def huge_premise(L):
    """each huge pixel is +-256 in every channel behind FromRGB's clamp, and every unit's float64 value is finite"""
    w = L.wants[f"encoder.b{L.cfg.resolution}.fromrgb"]
    for b, _, iy, ix, _ in HUGE_PIXELS:
        assert bool((w[b, :, iy, ix].abs() == 256.0).all()), (b, iy, ix)
    assert float((w.abs() == 256.0).double().mean()) < 0.01
    for name, v in L.wants.items():
        assert bool(torch.isfinite(v).all()), name
    return {}


BELOW2, ABOVE2, BELOW4 = 2.0 * (1 - 2.0 ** -13), 2.0 * (1 + 2.0 ** -13), 4.0 * (1 - 2.0 ** -13)


def _dressed(like, cfg, n, seed, styles, **kw):
    src = CASES[like]
    return _case(cfg, n, seed, env=src["env"], kernels=src["kernels"], dress=True, styles=styles, **kw)


# Seeds: each dressed case takes the smallest seed above the previous case's at which every noise strength of its forward (drawn
# N(0, 0.3^2), one per modulated layer of its resolution) is at least MIN_NOISE_STRENGTH; dressed_premise() asserts it.  The bound of
# a dressed unit is relative to 512, so the noise guard needs a strength of about 0.03 to see the term, and every seventh draw is
# smaller.  Skipped: 126, 128, 130, 132 (R16), 136-138, 140, 142, 143, 145 (R32), 147, 148 (R16).  r16_huge is not dressed: the next seed.
CASES.update({
    # two-plane operands on 64 columns: the clamp alone; mx exactly a power of two; mx just below and just above one, in two binades
    "r16_dress": _dressed("r16_const", R16, 3, 125, None),
    "r16_dress_t1": _dressed("r16_const", R16, 3, 127, 1.0),
    "r16_dress_below2": _dressed("r16_const", R16, 3, 129, BELOW2),
    "r16_dress_above2": _dressed("r16_const", R16, 3, 131, ABOVE2),
    "r16_dress_below4": _dressed("r16_const", R16, 3, 133, BELOW4),
    # the per-row noise epilogue on saturated values
    "r16_dress_t1_random": _dressed("r16_random", R16, 3, 134, 1.0, random_noise=True),
    # 256 columns, 16 x 16 tiles, accumulators in AGPRs
    "r16_c256_mti4_dress_below2": _dressed("r16_c256_mti4", R16W, 1, 135, BELOW2),
    # single-plane operands, and the fp16 loads and stores of +-512 and of saturated +-256
    "r32_f16_dress": _dressed("r32_f16", R32, 2, 139, None, flags=(8, 8)),
    "r32_f16_dress_below2": _dressed("r32_f16", R32, 2, 141, BELOW2, flags=(8, 8)),
    "r32_f16_st_dress": _dressed("r32_f16_st", R32, 2, 144, None, flags=(8, 8), storage=True),
    "r32_f16_st_dress_below2": _dressed("r32_f16_st", R32, 2, 146, BELOW2, flags=(8, 8), storage=True),
    # the per-sample scale read through the three per-image-operand kernels of an S-samples forward
    "r16_samples_dress_below2": _dressed("r16_samples", R16, 2, 149, BELOW2, samples=3),
    # one +inf, one -inf and one 3e38 pixel, in different images: +-256 behind FromRGB's clamp, finite from there on
    "r16_huge": _case(R16, 3, 150, kernels=CASES["r16_const"]["kernels"], huge=True),
})


def run_case(name, lib, mem, monkeypatch, report=None):
    c = CASES.get(name) or GPU_CASES[name]
    for k in ("COMODGAN_MTI", "COMODGAN_UP4", "COMODGAN_UP4_NT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    cfg = config(*c["cfg"])
    kw = dict(c["kw"])
    n, seed, s = c["n"], c["seed"], kw.get("samples", 1)
    sd = pkg.synth.make_comodgan_state_dict(cfg, seed)
    z = pkg.synth.make_latent(n * s, cfg.z_dim, seed)
    x = pkg.synth.make_input(n, cfg.resolution, seed)
    if kw.pop("random_noise", False):
        kw.update(noise_mode="random", noise=pkg.synth.normal((n * s * noise_floats(cfg),), seed, "layer-noise").astype(np.float32))
    if kw.pop("dress", False):
        styles = kw.pop("styles")
        sd, kw["premise"] = dress(cfg, sd, styles), dressed_premise(styles)
    if kw.pop("huge", False):
        for b, ch, iy, ix, v in HUGE_PIXELS:
            x[b, ch, iy, ix] = v
        kw["premise"] = huge_premise
    if kw.pop("bytes", False):
        from tests.comodgan_u8_case import make_u8
        kw["u8"], x = make_u8(n, cfg.resolution, seed), None
    rows, count = check_layers(lib, mem, cfg, sd, x, z, kernels=c["kernels"], tag=name, report=report, **kw)
    assert count == expected_units(cfg), (name, count, expected_units(cfg))
    return rows
