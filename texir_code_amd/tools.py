"""The asset step between IrT generation and material estimation (tools/padding_texture.py:49-87): zero texels of the
irradiance texture (seams / gutters) take the value of their nearest non-zero texel (Euclidean distance transform), so that
mip-mapped fetches near chart borders do not bleed black.  One-time CPU step in the reference (scipy + torch grid_sample); kept
on the same ops here, including grid_sample's nearest-rounding quirk.  The reference then pipes the padded texture through the
external Open Image Denoise binary (:86-87); `denoise_atrous` is a stand-in for that call (an edge-avoiding a-trous wavelet
filter, Dammertz et al. 2010, colour edge-stopping like OIDN's image-only mode, optionally guided by normal / position images) -- NOT a
re-implementation of OIDN's network.

What the quirk costs.  The reference's fill is NOT a nearest fill: F.grid_sample(mode="nearest") with the default align_corners=False
un-normalises source index i to i - 0.5 and rounds half to even, so every odd source row or column is read one texel too low -- and
that texel is often a hole again.  On seeded 96x128 and 100x124 atlases at 55 % occupancy `padding_texture` (= the reference, = mode
`reference` of the device route) leaves 33 % and 36 % of the hole texels black, and only a quarter of the holes with a unique nearest
texel receive that texel's value.  Mode `nearest` of the device route (texpost.pad_texture, csrc/texpost.hip) fills every hole from a
texel at minimal distance; `reference` reproduces this function bit for bit, for those who need the reference's file.

    python -m texir_code_amd.tools pad <.../0_irr_texture.hdr> [<.../irt.hdr>] [--denoise] [--gpu] [--mode nearest|reference]

Without --gpu: this module's CPU path (mode reference; --mode nearest needs --gpu).  With --gpu: texpost on the device, mode nearest unless told.

    python -m texir_code_amd.tools texel-gbuffer <.../out1.obj> <res> [<.../texel_gbuffer.npz>] [--normal geometric|shading]

The texel G-buffer of any uv-mapped mesh (position + 1e-2 * normal, normal; zero on the texels no triangle covers), rasterised in uv space on the
device (gbuffer.raster_texel_gbuffer) and written in the format train.texel_gbuffer = file reads.  <res> is the atlas size, or HxW.

    python -m texir_code_amd.tools bake-atlas <root> <res|HxW> [--out DIR] [--cos-min X] [--normal geometric|shading] [--seg]
                                              [--fill] [--fill-dist D] [--fill-cos C] [--query closest|any]

The radiance atlas hdr_texture.hdr and the index texture 0.png of <root>/vrproc/hdr_texture/out1.obj from the calibrated panoramas hdr/<id>/ccm.hdr
(info/aligned.txt, info/final_extrinsics.txt; the alpha of derived/<id>/panoImage_orig.jpg masks invalid pixels when it exists), selected per texel on the
device (atlas.bake_atlas, csrc/texbake.hip), written into DIR (default <root>/vrproc/hdr_texture/baked; existing files are not overwritten).  --seg adds
0_seg_gray.png gathered from derived/<id>/panoImage_gray.png.  --query any puts the segment test to the occlusion query (texir_atlas_bake_any) instead of a
closest-hit query (the default, closest): the files are the same, byte for byte.

--fill completes the atlas (atlas.fill_atlas, csrc/texfill.hip): a covered texel no panorama sees takes the radiance of the nearest OBSERVED texel in world
space within D scene units (--fill-dist, default 0.5: the depth of what stands on an indoor floor -- a choice, not a measurement) whose normal agrees with
its own to a cosine of C (--fill-cos, default 0.5); where nothing compatible is near it stays black.  Then the texels outside every chart take their
uv-nearest covered texel (atlas.dilate_gutters), so that bilinear footprints along chart borders read no black.  0.png keeps codes for OBSERVED texels only:
a filled texel is not seen by the view it borrows from, and under the `pano` G-buffer route its code would put it at the source's position; with
train.texel_gbuffer = raster the IrT stage computes irradiance at filled texels too.  atlas_fill.npz (src int32 [H,W], -1 elsewhere, file orientation) is
written beside the atlas so that later gathers can be completed the same way; with --seg a filled texel takes its source's class and gutters stay 0.
Without --fill every file is what the command wrote before the option existed, bit for bit.

    python -m texir_code_amd.tools relight-irt <dir> --class k --colour r,g,b [--replace]

From the files an IrT stage with train.irt_split wrote into <dir> (0_irr_texture_class<j>.hdr, the irradiance that comes from the texels of class j):
0_irr_texture_relit.hdr = sum_{j != k} E_j + colour * E_k -- class k's radiance scaled per channel (1,1,1 gives the plain texture back, 0,0,0 switches the
class off).  --replace: class k's texels become ONE colour instead, colour * 0_irr_texture_unit<k>.hdr (train.irt_split_unit; the reference's "lamp texels
become one colour", models/test_nvdiffrast.py:109-110).  Irradiance is linear in the radiance texture: nothing is traced.  Existing files are not overwritten.

    python -m texir_code_amd.tools light-irt <dir> --light k --colour r,g,b [--light j --colour r,g,b ...] [--base <file>] [--bounce] [--shadow] [--objects]

From the files an IrT stage with train.irt_lights wrote into <dir> (0_irr_texture_light<k>.hdr, the irradiance under inserted emitter k at unit radiance):
0_irr_texture_lit.hdr = base + sum colour_k * 0_irr_texture_light<k>.hdr -- the listed emitters switched on at those radiances.  Direct light only,
unless --bounce: then colour_k * 0_irr_texture_light<k>_bounce.hdr (train.irt_light_bounces: the new light's diffuse bounces) is added for every named
light as well.  The base is <dir>/0_irr_texture.hdr, or --base <file>, e.g. a 0_irr_texture_relit.hdr from relight-irt.  Irradiance is linear in emitted radiance: nothing is
traced.  --shadow: what the lamps' BODIES take from the base is subtracted first, floored at zero (train.irt_light_shadow: 0_irr_texture_lights_shadow.hdr, the
union of all bodies, when every light of the directory is named; 0_irr_texture_light<k>_shadow.hdr when one light is named; no other subset has a file).
--objects: the files with the inserted mesh objects in the way of the lamps' light take the plain ones' place (train.irt_light_objects:
0_irr_texture_light<k>_objects.hdr, and 0_irr_texture_light<k>_objects_bounce.hdr with --bounce); together with object-irt this gives the full relit atlas:
light-irt <dir> ... --objects --base <dir>/0_irr_texture_objects.hdr.  Existing files are not overwritten.

    python -m texir_code_amd.tools object-irt <dir> [--object k ...] [--base <file>]

From the files an IrT stage with train.irt_objects wrote into <dir> (0_irr_texture_object<k>_shadow.hdr, what inserted mesh object k takes from the
irradiance): 0_irr_texture_objects.hdr = max(base - lost, 0).  lost is 0_irr_texture_objects_shadow.hdr, the union of all objects, when every object of the
directory is named (or none is); 0_irr_texture_object<k>_shadow.hdr when one is named; no other subset has a file.  Nothing is traced.  Existing files are
not overwritten.
"""
import sys

import numpy as np
import torch
import torch.nn.functional as F

from . import io_formats as IO


def padding_texture(img):
    """img [H,W,3] float32 -> padded copy"""
    from scipy import ndimage
    img = np.asarray(img, np.float32)
    h, w, _ = img.shape
    mask = np.asarray((img[:, :, 0] + img[:, :, 1] + img[:, :, 2]) == 0.0, dtype=np.uint8)
    if mask.all():
        return img.copy()
    _, indices = ndimage.distance_transform_edt(mask, return_indices=True)
    indices = torch.from_numpy(indices).permute(1, 2, 0).reshape(-1, 2)
    img_t = torch.from_numpy(img).permute(2, 0, 1).unsqueeze(0)
    uv = torch.zeros((h * w, 2), dtype=torch.float32)
    m = torch.from_numpy(mask.reshape(-1).astype(bool))
    uv[m] = indices[m][:, [1, 0]].float() / torch.tensor([w, h]).unsqueeze(0) * 2.0 - 1.0
    res = F.grid_sample(img_t, uv.reshape(1, h, w, 2), mode="nearest", align_corners=False)[0].permute(1, 2, 0).numpy()
    mf = mask.astype(np.float32)[:, :, None]
    return res * mf + img * (1 - mf)


def denoise_atrous(img, iterations=3, sigma_c=0.5, device=None, guide_nrm=None, guide_pos=None, sigma_n=0.3, sigma_p=0.25):
    """edge-avoiding a-trous filter on log(1+x): `iterations` passes of the 5x5 B3-spline kernel with hole sizes 1, 2, 4, ... and the
    edge-stopping weight exp(-|dc|^2 / sigma_c^2) (sigma halves every pass).  Zero texels (unpadded seams) neither contribute nor change.
    guide_nrm / guide_pos [H,W,3] (optional) add |dn|^2 / sigma_n^2 and |dx|^2 / sigma_p^2 to the exponent (a sigma of 0 switches its term off; these
    two do not shrink with the pass; replicate border like the colour): the texel G-buffers tell the same surface from the unrelated chart across a gutter.
    Runs on `device` (default: the GPU when present); a 4k x 4k texture takes a few tens of milliseconds there.  texpost.denoise is the fused kernel."""
    if device is None:
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    x = torch.as_tensor(np.asarray(img, np.float32), device=device)
    valid = (x.sum(-1, keepdim=True) != 0).float()
    c = torch.log1p(x.clamp(min=0))
    k1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=device) / 16.0
    H, W, _ = c.shape
    guides = []
    for gimg, sg in ((guide_nrm, sigma_n), (guide_pos, sigma_p)):
        if gimg is not None and sg > 0:
            guides.append((torch.as_tensor(np.asarray(gimg, np.float32), device=device), sg ** 2))
    for it in range(iterations):
        step, s2 = 1 << it, (sigma_c * 0.5 ** it) ** 2
        acc, wsum = torch.zeros_like(c), torch.zeros((H, W, 1), device=device)
        pad = 2 * step
        rep = lambda t: F.pad(t.permute(2, 0, 1)[None], (pad, pad, pad, pad), mode="replicate")[0].permute(1, 2, 0)
        cp = rep(c)
        vp = F.pad(valid.permute(2, 0, 1)[None], (pad, pad, pad, pad), mode="constant", value=0.0)[0].permute(1, 2, 0)
        gp = [(gt, rep(gt), g2) for gt, g2 in guides]
        for dy in range(5):
            for dx in range(5):
                win = (slice(dy * step, dy * step + H), slice(dx * step, dx * step + W))
                q = cp[win]
                e = ((q - c) ** 2).sum(-1, keepdim=True) / s2
                for gt, gpad, g2 in gp:
                    e = e + ((gpad[win] - gt) ** 2).sum(-1, keepdim=True) / g2
                w = k1[dy] * k1[dx] * torch.exp(-e) * vp[win]
                acc += q * w
                wsum += w
        c = torch.where(valid > 0, acc / wsum.clamp(min=1e-20), c)
    return (torch.expm1(c) * valid).cpu().numpy()


def write_texel_gbuffer(path_obj, H, W, dst, normal="geometric", device=0):
    """out1.obj -> texel_gbuffer.npz (position, normal [H,W,3] float32 in file orientation); returns the number of covered texels"""
    from . import gbuffer as GB
    from .scene import Scene
    obj = IO.load_obj(path_obj)
    scene = Scene(obj["vertices"], obj["indices"], IO.triangle_uvs_open3d(obj), np.zeros((2, 2, 3), np.float32), device=device)     # (no radiance is read)
    if normal == "shading":
        GB.set_corner_normals(scene, IO.corner_normals(obj))
    pos, nrm, prim, _ = GB.raster_texel_gbuffer(scene, H, W, normal=normal, want_ids=True)
    np.savez(dst, position=pos.cpu().numpy(), normal=nrm.cpu().numpy())
    return int((prim >= 0).sum().item())


def parse_bake_atlas(argv):
    """the arguments after `bake-atlas` -> dict(root, H, W, out, cos_min, normal, seg, fill, fill_dist, fill_cos, query); ValueError names what is wrong"""
    opt = {"--out": None, "--cos-min": "0.1", "--normal": "geometric", "--fill-dist": "0.5", "--fill-cos": "0.5", "--query": "closest"}
    flags, rest = [], []
    it = iter(argv)
    for a in it:
        key = a.split("=", 1)[0]
        if key in opt:
            opt[key] = a.split("=", 1)[1] if "=" in a else next(it, None)
        elif a.startswith("--"):
            flags.append(a)
        else:
            rest.append(a)
    if len(rest) < 2:
        raise ValueError("bake-atlas needs <root> and <res|HxW>")
    try:
        hw = [int(v) for v in rest[1].lower().split("x")]
        H, W = (hw[0], hw[0]) if len(hw) == 1 else hw
        cm = float(opt["--cos-min"])
    except (ValueError, TypeError):
        raise ValueError("<res> must be an integer or HxW and --cos-min a number, got %r, %r" % (rest[1], opt["--cos-min"]))
    if opt["--normal"] not in ("geometric", "shading"):
        raise ValueError("--normal must be geometric or shading")
    if opt["--query"] not in ("closest", "any"):
        raise ValueError("--query must be closest or any, got %r" % (opt["--query"],))
    try:
        fd, fc = float(opt["--fill-dist"]), float(opt["--fill-cos"])
    except (ValueError, TypeError):
        raise ValueError("--fill-dist and --fill-cos must be numbers, got %r, %r" % (opt["--fill-dist"], opt["--fill-cos"]))
    if not fd > 0.0:
        raise ValueError("--fill-dist must be > 0, got %r" % fd)
    if not 0.0 <= fc <= 1.0:
        raise ValueError("--fill-cos must be in [0, 1], got %r" % fc)
    return {"root": rest[0], "H": H, "W": W, "out": opt["--out"], "cos_min": cm, "normal": opt["--normal"], "seg": "--seg" in flags, "fill": "--fill" in flags,
            "fill_dist": fd, "fill_cos": fc, "query": opt["--query"]}


def relight_irt(directory, k, colour, replace=False):
    """-> the path written.  FileExistsError / FileNotFoundError / ValueError name what is wrong"""
    import os
    from . import irtsplit
    dst = os.path.join(directory, "0_irr_texture_relit.hdr")
    if os.path.exists(dst):
        raise FileExistsError("%s exists: not overwritten" % dst)
    E = []
    while os.path.exists(os.path.join(directory, "0_irr_texture_class%d.hdr" % len(E))):
        E.append(np.asarray(IO.read_hdr(os.path.join(directory, "0_irr_texture_class%d.hdr" % len(E))), np.float32))
    if not E:
        raise FileNotFoundError("no 0_irr_texture_class0.hdr in %s: run the IrT stage with train.irt_split" % directory)
    if not 0 <= k < len(E):
        raise ValueError("--class %d: %s holds classes 0..%d" % (k, directory, len(E) - 1))
    E = np.stack(E)
    if replace:
        unit = os.path.join(directory, "0_irr_texture_unit%d.hdr" % k)
        if not os.path.exists(unit):
            raise FileNotFoundError("--replace needs %s: run the IrT stage with train.irt_split_unit = true" % unit)
        F = np.zeros_like(E)
        F[k] = IO.read_hdr(unit)
        out = irtsplit.replace_constant(E, F, k, colour)
    else:
        out = irtsplit.combine(E, [colour if j == k else 1.0 for j in range(len(E))])
    IO.write_hdr(dst, np.ascontiguousarray(out, np.float32))
    return dst


def light_irt(directory, lights, base=None, bounce=False, shadow=False, objects=False):
    """lights: [(k, (r, g, b)), ...]; bounce: also the lights' bounce files; shadow: the bodies' shadow on the base first; objects: the files with the
    inserted mesh objects in the way (train.irt_light_objects) in place of the plain ones -> the path written.
    FileExistsError / FileNotFoundError / ValueError name what is wrong"""
    import os
    from . import irtlight
    dst = os.path.join(directory, "0_irr_texture_lit.hdr")
    if os.path.exists(dst):
        raise FileExistsError("%s exists: not overwritten" % dst)
    base = os.path.join(directory, "0_irr_texture.hdr") if base is None else base
    if not os.path.exists(base):
        raise FileNotFoundError("no %s: run the IrT stage first, or name the base with --base" % base)
    if not lights:
        raise ValueError("light-irt needs at least one --light k --colour r,g,b")
    E = np.asarray(IO.read_hdr(base), np.float32)
    F = []
    for k, _ in lights:
        f = os.path.join(directory, "0_irr_texture_light%d%s.hdr" % (k, "_objects" if objects else ""))
        if k < 0 or not os.path.exists(f):
            if objects:
                raise FileNotFoundError("--light %d --objects needs %s: run the IrT stage with train.irt_light_objects = true (and train.irt_lights, "
                                        "train.irt_objects)" % (k, f))
            raise FileNotFoundError("--light %d needs %s: run the IrT stage with train.irt_lights = <json of the lights>" % (k, f))
        img = np.asarray(IO.read_hdr(f), np.float32)
        if img.shape != E.shape:
            raise ValueError("%s is %r, the base %s is %r" % (f, img.shape, base, E.shape))
        F.append(img[..., 0])
    lost = None
    if shadow:
        import re
        named = sorted(set(k for k, _ in lights))
        have = sorted(int(m.group(1)) for m in (re.fullmatch(r"0_irr_texture_light(\d+)\.hdr", n) for n in os.listdir(directory)) if m)
        if len(named) == 1:
            f = os.path.join(directory, "0_irr_texture_light%d_shadow.hdr" % named[0])
        elif named == have:
            f = os.path.join(directory, "0_irr_texture_lights_shadow.hdr")
        else:
            raise FileNotFoundError("--shadow of the lights %s: the stage writes the shadow of one lamp (0_irr_texture_light<k>_shadow.hdr) and of all %d "
                                    "together (0_irr_texture_lights_shadow.hdr), no other subset: name one light or all (train.irt_light_shadow = true)"
                                    % (named, len(have)))
        if not os.path.exists(f):
            raise FileNotFoundError("--shadow needs %s: run the IrT stage with train.irt_light_shadow = true (and train.irt_lights)" % f)
        lost = np.asarray(IO.read_hdr(f), np.float32)
        if lost.shape != E.shape:
            raise ValueError("%s is %r, the base %s is %r" % (f, lost.shape, base, E.shape))
    out = irtlight.add(E, np.stack(F), [c for _, c in lights], lost=lost)
    if bounce:
        G = []
        for k, _ in lights:
            f = os.path.join(directory, "0_irr_texture_light%d%s_bounce.hdr" % (k, "_objects" if objects else ""))
            if not os.path.exists(f):
                if objects:
                    raise FileNotFoundError("--bounce --objects needs %s: run the IrT stage with train.irt_light_objects = true and train.irt_light_bounces >= 1 "
                                            "(and train.irt_light_albedo)" % f)
                raise FileNotFoundError("--bounce needs %s: run the IrT stage with train.irt_light_bounces >= 1 (and train.irt_light_albedo)" % f)
            img = np.asarray(IO.read_hdr(f), np.float32)
            if img.shape != E.shape:
                raise ValueError("%s is %r, the base %s is %r" % (f, img.shape, base, E.shape))
            G.append(img)
        out = irtlight.add_indirect(out, np.stack(G), [c for _, c in lights])
    IO.write_hdr(dst, np.ascontiguousarray(out, np.float32))
    return dst


def main(argv):
    if len(argv) >= 2 and argv[0] == "object-irt":
        from . import irtobject
        rest, objects, base, bad = [], [], None, False
        it = iter(argv[1:])
        for a in it:
            key, eq, val = a.partition("=")
            if key in ("--object", "--base"):
                val = val if eq else next(it, None)
                try:
                    if key == "--object":
                        objects.append(int(val))
                    else:
                        if val is None or base is not None:
                            raise ValueError
                        base = val
                except (TypeError, ValueError):
                    bad = True
            elif a.startswith("--"):
                bad = True
            else:
                rest.append(a)
        if bad or len(rest) != 1 or any(k < 0 for k in objects):
            print("object-irt needs <dir> [--object k ...] [--base <file>]")
            return 2
        try:
            dst = irtobject.object_irt(rest[0], objects or None, base)
        except (FileExistsError, FileNotFoundError) as e:
            print(e)
            return 1
        except ValueError as e:
            print(e)
            return 2
        print("wrote", dst)
        return 0
    if len(argv) >= 2 and argv[0] == "light-irt":
        rest, lights, base, bad, bounce, shadow, objects = [], [], None, False, False, False, False
        it = iter(argv[1:])
        for a in it:
            key, eq, val = a.partition("=")
            if key in ("--light", "--colour", "--base"):
                val = val if eq else next(it, None)
                try:
                    if key == "--light":
                        lights.append([int(val), None])
                    elif key == "--colour":
                        colour = tuple(float(v) for v in val.split(","))
                        if len(colour) != 3 or not lights or lights[-1][1] is not None:
                            raise ValueError
                        lights[-1][1] = colour
                    else:
                        if val is None or base is not None:
                            raise ValueError
                        base = val
                except (TypeError, ValueError, AttributeError):
                    bad = True
            elif a == "--bounce":
                bounce = True
            elif a == "--shadow":
                shadow = True
            elif a == "--objects":
                objects = True
            elif a.startswith("--"):
                bad = True
            else:
                rest.append(a)
        if bad or len(rest) != 1 or not lights or any(c is None for _, c in lights):
            print("light-irt needs <dir> --light k --colour r,g,b [--light k --colour r,g,b ...] [--base <file>] [--bounce] [--shadow] [--objects]")
            return 2
        try:
            dst = light_irt(rest[0], [(k, c) for k, c in lights], base, bounce, shadow, objects)
        except (FileExistsError, FileNotFoundError) as e:
            print(e)
            return 1
        except ValueError as e:
            print(e)
            return 2
        print("wrote", dst)
        return 0
    if len(argv) >= 2 and argv[0] == "relight-irt":
        opt, rest, flags = {"--class": None, "--colour": None}, [], []
        it = iter(argv[1:])
        for a in it:
            key = a.split("=", 1)[0]
            if key in opt:
                opt[key] = a.split("=", 1)[1] if "=" in a else next(it, None)
            elif a.startswith("--"):
                flags.append(a)
            else:
                rest.append(a)
        try:
            k = int(opt["--class"])
            colour = tuple(float(v) for v in opt["--colour"].split(","))
            if len(rest) != 1 or len(colour) != 3 or any(f != "--replace" for f in flags):
                raise ValueError
        except (TypeError, ValueError, AttributeError):
            print("relight-irt needs <dir> --class k --colour r,g,b [--replace]")
            return 2
        try:
            dst = relight_irt(rest[0], k, colour, "--replace" in flags)
        except (FileExistsError, FileNotFoundError) as e:
            print(e)
            return 1
        except ValueError as e:
            print(e)
            return 2
        print("wrote", dst)
        return 0
    if len(argv) >= 3 and argv[0] == "bake-atlas":
        from . import atlas
        try:
            o = parse_bake_atlas(argv[1:])
        except ValueError as e:
            print(e)
            return 2
        try:
            res = atlas.bake_files(o["root"], o["H"], o["W"], o["out"], o["cos_min"], o["normal"], o["seg"], fill=o["fill"], fill_dist=o["fill_dist"],
                                   fill_cos=o["fill_cos"], query=o["query"])
        except FileExistsError as e:
            print(e)
            return 1
        print("wrote %s (%d x %d from %d panoramas of %d x %d): %.2f %% of %d covered texels got a view"
              % (res["dir"], o["H"], o["W"], res["view_count"], res["hw"][0], res["hw"][1], 100.0 * res["share"], res["covered"]))
        if o["fill"]:
            n = max(1, res["covered"])
            print("fill (dist %g, cos %g): %.2f %% of the covered texels observed, %.2f %% filled, %.2f %% left black"
                  % (o["fill_dist"], o["fill_cos"], 100.0 * res["observed"] / n, 100.0 * res["filled"] / n, 100.0 * res["black"] / n))
        return 0
    flags, rest, mode, normal = [], [], None, "geometric"
    out_dir, cos_min = None, "0.1"
    it = iter(argv)
    for a in it:
        if a in ("--out", "--cos-min") or a.startswith("--out=") or a.startswith("--cos-min="):
            key, val = a.split("=", 1) if "=" in a else (a, next(it, None))
            if key == "--out":
                out_dir = val
            else:
                cos_min = val
            continue
        if a == "--mode":
            mode = next(it, None)
        elif a.startswith("--mode="):
            mode = a.split("=", 1)[1]
        elif a == "--normal":
            normal = next(it, None)
        elif a.startswith("--normal="):
            normal = a.split("=", 1)[1]
        elif a.startswith("--"):
            flags.append(a)
        else:
            rest.append(a)
    argv = rest
    if len(argv) >= 3 and argv[0] == "texel-gbuffer":
        try:
            hw = [int(v) for v in argv[2].lower().split("x")]
            H, W = (hw[0], hw[0]) if len(hw) == 1 else hw
        except ValueError:
            print("<res> must be an integer or HxW, got %r" % argv[2])
            return 2
        if normal not in ("geometric", "shading"):
            print("--normal must be geometric or shading")
            return 2
        dst = argv[3] if len(argv) > 3 else argv[1].replace("out1.obj", "texel_gbuffer.npz") if "out1.obj" in argv[1] else "texel_gbuffer.npz"
        n = write_texel_gbuffer(argv[1], H, W, dst, normal)
        print("wrote %s (%d x %d, %d texels covered)" % (dst, H, W, n))
        return 0
    if len(argv) < 2 or argv[0] != "pad":
        print(__doc__)
        return 2
    gpu = "--gpu" in flags
    if mode is None:
        mode = "nearest" if gpu else "reference"
    if mode not in ("nearest", "reference") or (mode == "nearest" and not gpu):
        print("--mode must be nearest or reference; nearest needs --gpu (the CPU path is the reference's)")
        return 2
    src = argv[1]
    dst = argv[2] if len(argv) > 2 else src.replace("0_irr_texture", "irt")
    if gpu:
        from . import texpost
        dev = torch.from_numpy(np.ascontiguousarray(IO.read_hdr(src), np.float32)).cuda()
        dev = texpost.pad_texture(dev, mode=mode)
        if "--denoise" in flags:
            dev = texpost.denoise(dev)
        out = dev.cpu().numpy()
    else:
        out = padding_texture(IO.read_hdr(src))
        if "--denoise" in flags:
            out = denoise_atrous(out)
    IO.write_hdr(dst, out)
    print("wrote", dst)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
