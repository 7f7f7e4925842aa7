"""IrrTextureRunner -- drop-in for trainer/generate_ir_texture.py:31-82 (same kwargs, same output file)."""
import os
import sys

import numpy as np
import torch

from .. import io_formats as IO
from ..conf import ConfigFactory
from ..plugin import get_class
from ..runlog import phases


IRT_PAD = ("none", "nearest", "reference")
IRT_DENOISE = ("none", "color", "guided")


def irt_post_settings(conf):
    """the optional keys of the asset step between the stages (tools/padding_texture.py:49-87, run on the device by texpost):
      train.irt_pad = none (default: today's behaviour, no irt.hdr) | nearest (every zero texel from a texel at minimal distance) | reference (the
                      reference's grid_sample rounding bit for bit: about a third of the gutter texels stay black, tools.py);
      train.irt_denoise = none (default) | color | guided (a-trous filter, guided by the texel G-buffers); needs irt_pad != none;
      train.irt_denoise_sigma = [sigma_c, sigma_n, sigma_p] (default [0.5, 0.3, 0.25]).
    -> (pad, denoise, sigma); bad values raise ValueError."""
    pad = str(conf.get("train.irt_pad", "none")).lower()
    den = str(conf.get("train.irt_denoise", "none")).lower()
    if pad not in IRT_PAD:
        raise ValueError("train.irt_pad must be none, nearest or reference, got %r" % pad)
    if den not in IRT_DENOISE:
        raise ValueError("train.irt_denoise must be none, color or guided, got %r" % den)
    if den != "none" and pad == "none":
        raise ValueError("train.irt_denoise = %s needs train.irt_pad = nearest or reference (a denoised texture with black gutters is no irt.hdr)" % den)
    sigma = conf.get("train.irt_denoise_sigma", [0.5, 0.3, 0.25])
    try:
        sigma = tuple(float(v) for v in sigma)
    except (TypeError, ValueError):
        raise ValueError("train.irt_denoise_sigma must be a list of three numbers, got %r" % (sigma,))
    if len(sigma) != 3 or not sigma[0] > 0 or sigma[1] < 0 or sigma[2] < 0:
        raise ValueError("train.irt_denoise_sigma must be [sigma_c > 0, sigma_n >= 0, sigma_p >= 0], got %r" % (sigma,))
    return pad, den, sigma


class IrrTextureRunner:
    def __init__(self, **kwargs):
        torch.set_default_dtype(torch.float32)
        torch.set_num_threads(1)                 # as the reference's runners (e.g. trainer/train_material.py:34): host torch ops are tiny
        self.conf = ConfigFactory.parse_file(kwargs["conf"])
        self.irt_pad, self.irt_denoise, self.irt_denoise_sigma = irt_post_settings(self.conf)
        self.exps_folder_name = kwargs["exps_folder_name"]
        self.train_batch_size = self.conf.get_int("train.batch_size")
        self.nepochs = self.conf.get_int("train.mat_epoch")
        self.max_niters = kwargs["max_niters"]
        self.GPU_INDEX = kwargs["gpu_index"]
        # fix random seed (generate_ir_texture.py:45-47): the per-texel shifts come from this CPU generator
        torch.manual_seed(666)
        torch.cuda.manual_seed(666)
        np.random.seed(666)
        print("shell command : {0}".format(" ".join(sys.argv)))
        print("Loading data ...")
        with phases.phase("dataset", sync=False):
            self.train_dataset = get_class(self.conf.get_string("train.dataset_class"))(
                self.conf.get_string("train.path_mesh_open3d"), self.conf.get_list("train.pano_img_res"), self.conf.get_float("train.hdr_exposure"))
        print("Finish loading data ...")
        with phases.phase("model_init"):
            self.model = get_class(self.conf.get_string("train.model_class"))(
                conf=self.conf, ids=self.train_dataset.ids, extrinsics=self.train_dataset.extrinsics_list, optim_cam=self.conf.get_bool("train.optim_cam"))
            self.model.cuda()
        self.start_epoch = 0

    def run(self):
        print("generating...")
        irr_texture = self.model()
        target = self.conf.get_string("train.path_mesh_open3d").replace("out1.obj", "0_irr_texture.hdr")
        rank = int(os.environ.get("RANK", "0"))
        with phases.phase("download", sync=False):
            # pinned staging: the 4096^2 texture is 201 MB; a pageable .cpu() goes through the driver's bounce buffers at a fraction of the link rate
            host = torch.empty(irr_texture.shape, dtype=irr_texture.dtype, pin_memory=True)
            host.copy_(irr_texture)
            arr = host.numpy()
        print(arr.shape)
        if rank == 0:
            with phases.phase("write_hdr", sync=False):
                IO.write_hdr(target, arr)          # Radiance RGBE (RLE scanlines) like cv2.imwrite('.hdr') (generate_ir_texture.py:82)
            if self.irt_pad != "none":
                self._write_irt(irr_texture, target.replace("0_irr_texture.hdr", "irt.hdr"))
            # train.irt_split (models.TracerO3d): the irradiance per class of the texels it comes from, beside the plain file
            for what, split in (("class", getattr(self.model, "ir_split", None)), ("unit", getattr(self.model, "ir_split_unit", None))):
                if split is not None:
                    with phases.phase("write_hdr", sync=False):
                        for k in range(split.shape[0]):
                            IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_%s%d.hdr" % (what, k)), split[k].cpu().numpy())
            # train.irt_lights (models.TracerO3d): the unit-radiance irradiance of every inserted emitter, its factor in all three channels
            lights = getattr(self.model, "ir_lights", None)
            if lights is not None:
                with phases.phase("write_hdr", sync=False):
                    for k in range(lights.shape[0]):
                        IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_light%d.hdr" % k), lights[k][..., None].expand(-1, -1, 3).contiguous().cpu().numpy())
            # train.irt_light_bounces (models.TracerO3d): the diffuse bounces of every inserted emitter's light at unit radiance, beside its direct file
            bounce = getattr(self.model, "ir_lights_bounce", None)
            if bounce is not None:
                with phases.phase("write_hdr", sync=False):
                    for k in range(bounce.shape[0]):
                        IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_light%d_bounce.hdr" % k), bounce[k].contiguous().cpu().numpy())
            # train.irt_light_objects (models.TracerO3d): the same two kinds of file with the inserted objects in the way of the lamps' light
            lights_obj, bounce_obj = getattr(self.model, "ir_lights_objects", None), getattr(self.model, "ir_lights_objects_bounce", None)
            if lights_obj is not None:
                with phases.phase("write_hdr", sync=False):
                    for k in range(lights_obj.shape[0]):
                        IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_light%d_objects.hdr" % k),
                                     lights_obj[k][..., None].expand(-1, -1, 3).contiguous().cpu().numpy())
                    if bounce_obj is not None:
                        for k in range(bounce_obj.shape[0]):
                            IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_light%d_objects_bounce.hdr" % k), bounce_obj[k].contiguous().cpu().numpy())
            # train.irt_light_shadow (models.TracerO3d): what every inserted emitter's body takes from the irradiance, and all of them together
            shadow, shadow_all = getattr(self.model, "ir_lights_shadow", None), getattr(self.model, "ir_lights_shadow_all", None)
            if shadow is not None:
                with phases.phase("write_hdr", sync=False):
                    for k in range(shadow.shape[0]):
                        IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_light%d_shadow.hdr" % k), shadow[k].contiguous().cpu().numpy())
                    if shadow_all is not None:
                        IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_lights_shadow.hdr"), shadow_all.contiguous().cpu().numpy())
            # train.irt_objects (models.TracerO3d): what every inserted mesh object takes from the irradiance, and all of them together
            shadow, shadow_all = getattr(self.model, "ir_objects_shadow", None), getattr(self.model, "ir_objects_shadow_all", None)
            if shadow is not None:
                with phases.phase("write_hdr", sync=False):
                    for k in range(shadow.shape[0]):
                        IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_object%d_shadow.hdr" % k), shadow[k].contiguous().cpu().numpy())
                    if shadow_all is not None:
                        IO.write_hdr(target.replace("0_irr_texture.hdr", "0_irr_texture_objects_shadow.hdr"), shadow_all.contiguous().cpu().numpy())
        return irr_texture

    def _write_irt(self, irr_texture, path):
        """the Mat stage's irt.hdr (models.py: MaterialModel reads it) from the assembled device texture: what tools/padding_texture.py:49-87 does to the
        file between the stages.  Rank 0 only -- every rank holds the whole texture, no collective is added.  Holes are judged on the image (zero texels),
        not on the seam mask: that is what the reference does to the file."""
        from .. import texpost
        with phases.phase("irt_post"):
            want_src = self.irt_denoise == "guided"
            res = texpost.pad_texture(irr_texture, mode=self.irt_pad, return_src=want_src)
            if self.irt_denoise == "color":
                res = texpost.denoise(res, sigma=self.irt_denoise_sigma)
            elif self.irt_denoise == "guided":
                res, src = res
                nrm = texpost.gather_src(self.model.normal_texture, src)
                pos = texpost.gather_src(self.model.position_texture, src)
                res = texpost.denoise(res, nrm=nrm, pos=pos, sigma=self.irt_denoise_sigma)
            host = torch.empty(res.shape, dtype=res.dtype, pin_memory=True)
            host.copy_(res)
            IO.write_hdr(path, host.numpy())
