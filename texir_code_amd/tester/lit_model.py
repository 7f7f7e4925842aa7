"""The evaluation model with inserted lamps: tester.test_model.MaterialModel plus one conf key the reference does not have.

    test.lights = none | <json of inserted emitters, the file form of train.irt_lights (irtlight.load)>
    test.light_samples = 64
    test.light_bounces = 0            diffuse bounces of the new light (irtlight.bounce), gathered once at construction on the irradiance texture's grid
    test.light_bounce_samples = 256   samples per texel and bounce
    test.light_shadows = false        the shadow the lamps' bodies cast on the captured diffuse light (Scene.irt_shadow), traced once at construction
    test.light_shadow_samples = 256   samples per texel
    test.objects = none               | <irtobject list or json, the form of train.irt_objects>: inserted mesh objects that shadow the lamps' light
    test.spec_shadows = false         the shadow the lamps' bodies and the objects cast in the SPECULAR term of the captured light (Scene.spec_shadow), per view

With lights, render() adds their diffuse and specular response to every rendered view, sum_k colour_k (albedo / pi F[k] + R[k]) (Scene.irt_lights,
Scene.spec_lights, irtlight.add_view), at test.light_samples samples per pixel, light and technique, with the pixels' own specular shift and the model's
floor of denominators.  With test.light_bounces >= 1 the model also builds, once, a texel G-buffer of irt.hdr's size, the lights' factors F per texel, and
G = irtlight.bounce(...) with the albedo texture as the diffuse albedo; it keeps sum_k colour_k G[k] as a texture in file orientation, forward() fetches
it with the very call that fetches the irradiance texture, and render() adds albedo / pi times that.  The texel shifts come from a private generator with a
fixed seed: the CPU generator's stream stays what it is.  With test.light_shadows the model builds, once and on the same texel G-buffer with the same
private generator, `lost`: what the union of the lamps' bodies takes from the captured irradiance; forward() fetches it like the irradiance texture and
render() takes albedo / pi * (irr - max(irr - lost, 0)) from the diffuse term before the lamps' light is added (irtlight.add_view(lost=, irr=)).
With test.objects (it needs test.lights) the objects are loaded once (irtobject.load) and handed to the irt_lights and spec_lights calls of render()
and to the F that seeds the bounce: the lamps' diffuse and specular light is shadowed by the objects (Scene.irt_lights(occluders=...)).  Not computed with
objects: the bounce's own rays (they still ignore the objects), their shadow on captured DIFFUSE light on the room's pixels.
    test.draw_objects = false         true (it needs test.objects, and so test.lights): the objects are DRAWN in the view
    test.object_materials = none      | <list of { "albedo": g | [r, g, b], "roughness": r }, one per object, or a json of one> (irtobject.materials; 0.5, 0.5)
    test.object_samples = 256         samples per object pixel of its captured irradiance
With test.draw_objects the view's G-buffer is the instanced one (gbuffer.cast_gbuffer(occluders=...), cached per view): a pixel shows the nearest of the room
and the objects, forward() also returns inst_id and empty_mask is 1 on object pixels.  On the pixels with inst_id = j >= 0 render() substitutes its inputs
before it calls the base, after any editing recolouring (a seg fetched at uv 0 cannot repaint an object): albedo and roughness are object j's material, irr
= max(E - lost, 0) with E = Scene.irt_generate at the pixel and lost = Scene.irt_shadow_mesh over all instances as one set (the captured light the object
itself and its neighbours intercept), at test.object_samples samples with shifts from a private generator with a fixed seed; the fetched bounce and
light-shadow terms are 0 there (their uv is not a surface of the atlas).  Everything after that is the code that runs on every pixel: the lamps' F and R use
the objects as occluders, spec_shadow applies if on, add_view composes -- so the objects are lit and shadowed by the inserted lamps.  Not computed with
drawn objects: the lamps' bodies drawn in the view; bounce light onto objects; the objects' own shadow on the captured SPECULAR term unless
test.spec_shadows is on; under relighting=True the base re-traces the diffuse term of every pixel against the room alone, so the objects' own shadow on
that term is missing there; textured objects (occluders have no uvs).
With test.spec_shadows (it needs test.lights) render() traces, per view and on the pixels' own replayed specular shift, what the union of the lamps' bodies
and of the objects takes from the specular term of the captured light (Scene.spec_shadow at the model's own sample count and floor of denominators, one
set holding all of them) and irtlight.add_view(lost_spec=) takes it from the pixel first, floored at zero.
Not computed: bodies shadowing each other's light, the body drawn in the view, a specular bounce, the specular shadow on the bounce's own rays.
With the default `none` the class IS its base: every file Editing, View, Relighting and Error write is unchanged byte for byte.
This is the class the plugin registry hands the tester runners for models.test_nvdiffrast.MaterialModel."""
import torch

from .. import gbuffer as GB, irtlight, irtobject, texpost
from ..texture import texture as tex_fetch
from . import test_model as TM

BOUNCE_SEED = 20241                       # the private generator of the texel shifts
OBJECT_SEED = 20242                       # the private generator of the object pixels' irradiance shifts


def load_test_lights(spec, device):
    """test.lights: 'none' -> None; a json path (irtlight.load) -> (records [K,16], colours [K,3]) on the device"""
    if spec.lower() == "none":
        return None
    records, colours = irtlight.load(spec)
    return torch.from_numpy(records).to(device), torch.from_numpy(colours).to(device)


def load_test_objects(spec, lights, device):
    """test.objects: none -> None; an irtobject list or json (the form of train.irt_objects) -> the keywords Scene.irt_lights / spec_lights take:
    {occluders, instances, poses}, loaded once.  It needs test.lights: a ValueError names both keys"""
    try:
        objects = irtobject.parse(spec)
    except (ValueError, FileNotFoundError) as e:
        raise type(e)(str(e).replace(irtobject.KEY, "test.objects"))
    if objects is None:
        return None
    if lights is None:
        raise ValueError("test.objects needs test.lights = <json of the lights>: the objects shadow the inserted emitters' light")
    occluders, inst, poses = irtobject.load(objects, device=device)
    return {"occluders": occluders, "instances": inst, "poses": poses}


def light_bounce_settings(conf):
    """test.light_bounces (0) and test.light_bounce_samples (256) -> (bounces >= 0, samples >= 1); bad values raise ValueError"""
    out = []
    for key, default, least in (("test.light_bounces", 0, 0), ("test.light_bounce_samples", 256, 1)):
        v = conf.get(key, default)
        try:
            if isinstance(v, bool) or int(v) != float(v) or int(v) < least:
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("%s must be an integer >= %d, got %r" % (key, least, v))
        out.append(int(v))
    return tuple(out)


def light_shadow_settings(conf):
    """test.light_shadows (false) and test.light_shadow_samples (256) -> (on, samples >= 1); bad values raise ValueError"""
    on = conf.get("test.light_shadows", False)
    if not isinstance(on, bool):
        raise ValueError("test.light_shadows must be true or false, got %r" % (on,))
    v = conf.get("test.light_shadow_samples", 256)
    try:
        if isinstance(v, bool) or int(v) != float(v) or int(v) < 1:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("test.light_shadow_samples must be an integer >= 1, got %r" % (v,))
    return on, int(v)


def spec_shadow_setting(conf, lights):
    """test.spec_shadows (false) -> bool; anything but true / false raises ValueError, and so does true without test.lights (the message names both keys)"""
    on = conf.get("test.spec_shadows", False)
    if not isinstance(on, bool):
        raise ValueError("test.spec_shadows must be true or false, got %r" % (on,))
    if on and lights is None:
        raise ValueError("test.spec_shadows needs test.lights = <json of the lights>: the lamps' bodies (and test.objects) cast the shadow")
    return on


def draw_objects_settings(conf, objects):
    """test.draw_objects (false), test.object_materials (none) and test.object_samples (256) -> (on, (albedo [K,3], roughness [K]) float32 or None, samples
    >= 1).  true needs test.objects, and so test.lights: the ValueError names the keys.  Off: the materials are not read"""
    on = conf.get("test.draw_objects", False)
    if not isinstance(on, bool):
        raise ValueError("test.draw_objects must be true or false, got %r" % (on,))
    if on and objects is None:
        raise ValueError("test.draw_objects needs test.objects = <list of {obj, pose}> (and so test.lights = <json of the lights>): the objects are what is drawn")
    v = conf.get("test.object_samples", 256)
    try:
        if isinstance(v, bool) or int(v) != float(v) or int(v) < 1:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("test.object_samples must be an integer >= 1, got %r" % (v,))
    mats = irtobject.materials(conf.get("test.object_materials", "none"), len(objects["instances"])) if on else None
    return on, mats, int(v)


class MaterialModel(TM.MaterialModel):
    def __init__(self, conf, *args, **kwargs):
        super().__init__(conf, *args, **kwargs)
        self.test_lights = load_test_lights(str(conf.get("test.lights", "none")), self.device)
        self.light_samples = int(conf.get("test.light_samples", 64))
        self.test_objects = load_test_objects(conf.get("test.objects", "none"), self.test_lights, self.device)
        self.light_bounces, self.light_bounce_samples = light_bounce_settings(conf)
        self.bounce_tex = None
        self.light_shadows, self.light_shadow_samples = light_shadow_settings(conf)
        self.shadow_tex = None
        self.spec_shadows = spec_shadow_setting(conf, self.test_lights)
        self.draw_objects, mats, self.object_samples = draw_objects_settings(conf, self.test_objects)
        if self.draw_objects:
            self.object_albedo, self.object_roughness = (torch.from_numpy(m).to(self.device) for m in mats)
        if self.test_lights is not None and self.light_bounces >= 1:
            self.build_bounce_texture()
        if self.test_lights is not None and self.light_shadows:
            self.build_shadow_texture()

    def _texel_inputs(self):
        """the texel G-buffer of the irradiance texture's grid and the texel shifts of the private generator: (H, W, pos, nrm, shift, ids, covered)"""
        H, W = int(self.irrt.shape[0]), int(self.irrt.shape[1])
        pos, nrm, prim, _ = GB.raster_texel_gbuffer(self.scene, H, W, normal="geometric", offset=1e-2, want_ids=True)
        covered = (prim >= 0).reshape(-1)
        ids = torch.nonzero(covered)[:, 0].to(torch.int32)
        gen = torch.Generator().manual_seed(BOUNCE_SEED)
        shift = torch.rand(H * W, 2, generator=gen).to(self.device)
        return H, W, pos.reshape(-1, 3).contiguous(), nrm.reshape(-1, 3).contiguous(), shift, ids, covered

    def build_shadow_texture(self):
        """what the union of the lamps' bodies takes from the captured irradiance, on the irradiance texture's grid, file orientation
        -> self.shadow_tex [H,W,3] (device)"""
        records, _ = self.test_lights
        H, W, pos, nrm, shift, ids, _ = self._texel_inputs()
        lost = self.scene.irt_shadow(pos, nrm, shift, int(self.light_shadow_samples), records, sets=[list(range(records.shape[0]))], texel_ids=ids)
        self.shadow_tex = lost[0].reshape(H, W, 3).contiguous()
        return self.shadow_tex

    def build_bounce_texture(self):
        """sum_k colour_k G[k] on the irradiance texture's grid, file orientation -> self.bounce_tex [H,W,3] (device)"""
        records, colours = self.test_lights
        H, W, pos, nrm, shift, ids, covered = self._texel_inputs()
        F = self.scene.irt_lights(pos, nrm, shift, records, int(self.light_samples), texel_ids=ids, **(getattr(self, "test_objects", None) or {})).reshape(-1, H, W)
        src = None
        if (H, W) == tuple(self.scene.tex_shape[:2]):
            src = texpost.pad_texture(covered.reshape(H, W, 1).to(torch.float32), return_src=True)[1]
        albedo = self.materials_a.detach().to(self.device)                  # file orientation, as irt.hdr: forward() fetches both with one uv
        G = irtlight.bounce(self.scene, pos, nrm, shift, albedo, F, int(self.light_bounce_samples), bounces=int(self.light_bounces), texel_ids=ids,
                            hw=(H, W), src=src).reshape(-1, H, W, 3)
        self.bounce_tex = irtlight.add_indirect(torch.zeros((H, W, 3), device=self.device), G, colours).contiguous()
        return self.bounce_tex

    def _gbuffer(self, mvp, view_id):
        """with test.draw_objects the instanced G-buffer of the loaded objects (gbuffer.cast_gbuffer(occluders=...)), cached per view as the base's is"""
        if not getattr(self, "draw_objects", False):
            return super()._gbuffer(mvp, view_id)
        key = (str(view_id), hash(mvp.cpu().numpy().tobytes()))
        gb = self._gb_cache.get(key)
        if gb is None:
            gb = GB.cast_gbuffer(self.scene, mvp, self.cube_res, flip_v=True, **self.test_objects)
            self._gb_cache[key] = gb
        return gb

    def forward(self, mvp, id, cam_position, *args, **kwargs):
        if getattr(self, "draw_objects", False):
            return self._forward_drawn(mvp, id, cam_position, *args, **kwargs)
        tex, sh = getattr(self, "bounce_tex", None), getattr(self, "shadow_tex", None)
        if tex is None and sh is None:
            return super().forward(mvp, id, cam_position, *args, **kwargs)
        gb = self._gbuffer(mvp, id)                                          # (cached: the base's own call below gets the same G-buffer)
        if tex is not None:
            self._bounce_irr = tex_fetch(tex, gb["uv"], gb["uv_da"], "linear-mipmap-linear", self.max_mip_level)
        if sh is not None:
            self._shadow_irr = tex_fetch(sh, gb["uv"], gb["uv_da"], "linear-mipmap-linear", self.max_mip_level)
        try:
            return super().forward(mvp, id, cam_position, *args, **kwargs)
        finally:
            self._bounce_irr = self._shadow_irr = None

    def _forward_drawn(self, mvp, id, cam_position, *args, **kwargs):
        """forward() with test.draw_objects: the base's forward on the instanced G-buffer; render() below learns which pixels show an object from
        self._inst_id and substitutes their inputs.  The result also has inst_id [6,c,c]; empty_mask is the G-buffer's mask, 1 on object pixels"""
        gb = self._gbuffer(mvp, id)
        tex, sh = getattr(self, "bounce_tex", None), getattr(self, "shadow_tex", None)
        on_obj = (gb["inst_id"] >= 0).unsqueeze(-1)
        # the fetched bounce and light-shadow terms are zero on object pixels: their uv is not a surface of the atlas
        if tex is not None:
            self._bounce_irr = torch.where(on_obj, 0.0, tex_fetch(tex, gb["uv"], gb["uv_da"], "linear-mipmap-linear", self.max_mip_level))
        if sh is not None:
            self._shadow_irr = torch.where(on_obj, 0.0, tex_fetch(sh, gb["uv"], gb["uv_da"], "linear-mipmap-linear", self.max_mip_level))
        self._inst_id = gb["inst_id"]
        try:
            res = super().forward(mvp, id, cam_position, *args, **kwargs)
        finally:
            self._bounce_irr = self._shadow_irr = self._inst_id = None
        res["inst_id"] = gb["inst_id"]
        return res

    def object_inputs(self, inst_id, normal, albedo, roughness, points, irr):
        """the inputs of render() with the object pixels (inst_id = j >= 0) substituted: albedo and roughness are object j's material; irr = max(E - lost, 0)
        with E = Scene.irt_generate at the pixel's point and normal and lost = Scene.irt_shadow_mesh over ALL instances as one set -- the captured light the
        object itself and its neighbours intercept -- both at test.object_samples samples with shifts from a private generator (the CPU generator's stream
        stays what it is) -> (albedo, roughness, irr), shaped as given"""
        P = normal.numel() // 3
        ids = torch.nonzero(inst_id.reshape(P) >= 0)[:, 0]
        if ids.numel() == 0:
            return albedo, roughness, irr
        j = inst_id.reshape(P)[ids].long()
        alb, rgh, ir = albedo.reshape(P, 3).clone(), roughness.reshape(P).clone(), irr.reshape(P, 3).clone()
        alb[ids], rgh[ids] = self.object_albedo[j], self.object_roughness[j]
        gen = torch.Generator().manual_seed(OBJECT_SEED)
        shift_o = torch.rand(P, 2, generator=gen).to(self.device)
        pts, nrm = points.reshape(P, 3).contiguous(), normal.reshape(P, 3).contiguous()
        N = int(self.object_samples)
        E = self.scene.irt_generate(pts, nrm, shift_o, N, texel_ids=ids.to(torch.int32))
        J = len(self.test_objects["instances"])
        lost = self.scene.irt_shadow_mesh(pts, nrm, shift_o, N, sets=[list(range(J))], texel_ids=ids.to(torch.int32), **self.test_objects)[0]
        ir[ids] = torch.clamp(E[ids] - lost[ids], min=0.0)
        return alb.reshape(albedo.shape), rgh.reshape(roughness.shape), ir.reshape(irr.shape)

    def render(self, normal, albedo, roughness, points, cam_position, irr):
        inst_id = getattr(self, "_inst_id", None)
        if inst_id is not None:                                              # (test.draw_objects: after any editing recolouring, before the base)
            albedo, roughness, irr = self.object_inputs(inst_id, normal, albedo, roughness, points, irr)
        lights = getattr(self, "test_lights", None)
        if lights is None:
            return super().render(normal, albedo, roughness, points, cam_position, irr)
        # The base draws the pixels' specular shift from the CPU generator and keeps it to itself.  The same numbers are drawn again from a private
        # generator started at the state the base found: the CPU generator itself sees the base's draws and no further one.
        replay = torch.Generator()
        replay.set_state(torch.get_rng_state())
        res = super().render(normal, albedo, roughness, points, cam_position, irr)
        shape = tuple(normal.shape[:-1])
        P = normal.numel() // 3
        if self.relighting:
            torch.rand(P, 1, 2, generator=replay)                                        # the diffuse term's draw comes first (test_model.render)
        shift_s = torch.rand(P, 1, 2, generator=replay).reshape(P, 2).to(self.device)
        records, colours = lights
        n_l = int(getattr(self, "light_samples", 64))
        pts, nrm, alb = points.reshape(P, 3), normal.reshape(P, 3), albedo.reshape(P, 3)
        objects = getattr(self, "test_objects", None) or {}                  # (none: the calls are the ones they were)
        F = self.scene.irt_lights(pts, nrm, shift_s, records, n_l, **objects)
        R = self.scene.spec_lights(pts, nrm, roughness.reshape(P), shift_s, cam_position, records, n_l, clamp_eps=TM.TINY_NUMBER, **objects)
        G, lost = getattr(self, "_bounce_irr", None), getattr(self, "_shadow_irr", None)
        spec = {}                                                            # (off: the calls are the ones they were)
        if getattr(self, "spec_shadows", False):
            spec["lost_spec"] = self.scene.spec_shadow(pts, nrm, roughness.reshape(P), shift_s, cam_position, int(self.sample_l[1]), bodies=records,
                                                       clamp_eps=TM.TINY_NUMBER, **objects)[0]
        if lost is None:
            res["rgb"] = irtlight.add_view(res["rgb"].reshape(P, 3), alb, F, R, colours, G=None if G is None else G.reshape(P, 3), **spec).reshape(shape + (3,))
        else:
            res["rgb"] = irtlight.add_view(res["rgb"].reshape(P, 3), alb, F, R, colours, G=None if G is None else G.reshape(P, 3), lost=lost.reshape(P, 3),
                                           irr=irr.reshape(P, 3), **spec).reshape(shape + (3,))
        return res
