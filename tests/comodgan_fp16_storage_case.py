"""Shared by the emulator and GPU tests of fp16 activation storage in Co-Mod-GAN's half-precision blocks
(include/comodgan_fp16_storage_hip.h): which blocks a pair of flags marks, and the check of a launch list against the tensor rule."""
F16, CONV_H = "cm_conv_f16_kernel", "cm_conv_h_kernel"
TYPED = ("cm_conv_h_kernel", "cm_fir_h_kernel", "cm_fir_samples_h_kernel", "cm_fromrgb_h_kernel", "cm_torgb_h_kernel")


def blocks(cfg, flags):
    """(marked encoder resolutions, marked synthesis resolutions) as the reference marks them (comodgan.py:148,384)"""
    res = [2 ** k for k in range(3, cfg.resolution.bit_length())]
    return ({r for r in res if flags[0] is not None and r > flags[0]}, {r for r in res if flags[1] is not None and r > flags[1]})


def check_storage_names(info, info_ops, cfg, flags):
    """info: the launch list with storage on; info_ops: the operand-only list of the same flags and forced forms"""
    enc, syn = blocks(cfg, flags)
    first = min(syn) if syn else None
    assert [i["layer"] for i in info] == [i["layer"] for i in info_ops]
    seen = set()
    for i, o in zip(info, info_ops):
        layer, k = i["layer"], i["kernel"]
        net, block = layer.split(".")[:2]
        r = int(block[1:]) if block[1:].isdigit() else 0
        mk = r > 4 and r in (enc if net == "encoder" else syn)
        if layer.endswith((".wprep", ".split")) or net not in ("encoder", "synthesis") or r <= 4:
            assert k == o["kernel"], (layer, k)
        elif "cm_conv" in o["kernel"]:
            keeps = not mk or (net == "synthesis" and r == first and ".conv0" in layer)     # the first marked block's transposed launches
            assert (k == o["kernel"]) if keeps else (CONV_H in k), (layer, k)
            if mk and keeps:
                assert F16 in k
            if CONV_H in k:
                # fp16 in, fp32 out only where the last marked encoder block hands over to an fp32 block
                last = net == "encoder" and ".conv1" in layer and (r // 2) not in enc
                assert k.endswith(", false>" if last else ", true>"), (layer, k)
        elif layer.endswith(".fir") and net == "encoder":
            assert k == ("migan::cm_fir_h_kernel<0, true, true, false>" if mk else o["kernel"]), (layer, k)
        elif layer.endswith(".fir"):
            xh, yh, sh = mk and r != first, mk, r in enc
            name = "cm_fir_samples_h_kernel<" if "samples" in o["kernel"] else "cm_fir_h_kernel<1, "
            want = f"migan::{name}{str(xh).lower()}, {str(yh).lower()}, {str(sh).lower()}>" if (xh or yh or sh) else o["kernel"]
            assert k == want, (layer, k, want)
        elif layer.endswith(".fromrgb"):
            assert k == ("migan::cm_fromrgb_h_kernel" if mk else o["kernel"]), (layer, k)
        elif layer.endswith(".torgb"):
            assert k == (o["kernel"].replace("cm_torgb_kernel", "cm_torgb_h_kernel") if mk else o["kernel"]), (layer, k)
        else:
            assert k == o["kernel"], (layer, k)
        seen |= {t for t in TYPED if t + "<" in k or k.endswith(t)}
    return seen
