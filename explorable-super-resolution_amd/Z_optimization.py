"""Latent-space (Z) optimisation through the frozen generator — the loop of the reference's codes/Z_optimization.py
(Optimizable_Z :273-319, Z_optimizer.optimize :647-797): tanh-bounded Z parameter, Adam, per iteration
    Z = Z_range*tanh(P)  ->  model.feed_data({'LR', 'Z'})  ->  model.test(prevent_grads_calc=False)   (G + CEM forward WITH graph,
    weights frozen)  ->  clamp(0,1)  ->  objective  ->  loss.mean().backward()  (data-gradient kernels only)  ->  Adam step,
keeping the iterate with the smallest loss.  The forward/backward are the HIP kernels; the objectives are element-wise / reduction torch ops
and the library's objective kernels on the SR output.  Every accepted objective name is one entry of the table OBJECTIVES in Z_objectives.py; its family's
class says what it computes, with the reference's lines, what it is fed and what it refuses (STD, Distance, Histogram, Periodicity,
PatchMagnitude, Scribble, Random).  The name is read once, by resolve(), at construction.  All of them run
whole-image or restricted to a user-marked region (image_mask: where the objective looks; Z_mask: which latent entries may move — the GUI's
region tools, GUI.py:1925-2057), except 'l1' and the VGG names, which take no masks.
The region constraint (non_local_Z_optimization on a partial image mask; 'scribble', the patch-magnitude and the periodicityPlus names): the
rebuilt Z mask and w x l1(out (1 - lm), initial (1 - lm)) on esr_hip.scribble.region_constraint, w the family's.
Not part of this build (NotImplementedError): 'random_VGG_limited' (the reference subtracts an image from a feature map), the random names with
'local' (the GUI's LIMITED_RANDOM_WITH_STD_NOT_L1, off as shipped), the random objectives in training mode (HR_unpadder) and 'random_VGG' with
masks; the GUI's adversarial objectives, 'scribble' without an image mask (the reference's plain-L1
fallback, which the GUI never sends: use 'l1'), the 'Plus' / 'Mag' spellings other than the six names of PLUS_OBJECTIVES and MAG_OBJECTIVES,
the other 'local_*' names without STD (the overlap-0.5 patch selection with its non-covered pixels), the local / periodicity / scribble /
patch-magnitude objectives in training mode (HR_unpadder), the region constraint (non_local_Z_optimization on a partial image mask) for any
objective but 'scribble' and those six names (the other local and periodicity ones refuse it, the whole-image ones ignore it), the '*_localSTD'
histogram variants and the automatic histogram temperature.  The refusals by name are the ordered list REFUSALS.
JPEG mode (jpeg_extractor given; models/DecompCNN_model.py): the model's fake_H holds DCT coefficients and its image is output_image (0...255),
Z lives on the block grid (Z_size = [H/8, W/8]) and data carries 'Uncomp' or 'Comp' and 'QF' (or a JPEG file's 'Q_table', and for the colour
model its 'compressed_chroma': esr_hip.jpeg_file.JpegFile.model_data) in place of 'LR'.  Accepted on either model (JPEG_OBJECTIVES): 'l1',
'TV', 'max_STD', 'min_STD', 'STD_increase', 'STD_decrease'.  On a colour model (chroma_mode) Z_size is still the Y grid, the objectives see the RGB
output, Z's gradient runs through both generators, and a model fed with the Y coefficients as 'Comp' gets data['uncompressed_chroma']
([B, 2, H, W] Cb, Cr) passed to model.test.  The colour model (the one the reference's JPEG GUI builds) also takes the editing objectives
(JPEG_EDIT_OBJECTIVES): the local-STD, periodicity, periodicityPlus and patch-magnitude names, 'scribble', 'hist' and the patch-histogram /
dictionary names, 'random_l1' and 'random_l1_limited'.  The reference evaluates all of them on model.Output_Batch(within_0_1=True) whatever
the model (:617, :680); so here: an
objective's value in JPEG mode is, by definition, its SR-mode value on model.Output_Image_0_1() (the un-clamped RGB image in 0...1, csrc/
esr_jpeg_edit.hip's esr_ycbcr_rgb on the GPU) in place of fake_H, the clamp inside the kernels as there.  The region constraint takes its
block-grid form (:355-357): Z mask = min(1, E + D), E = 1 inside a margin of 24 // 8 blocks, D the 8 x 8 block maximum of dilate16(image_mask).
The caller smears the scribble mask to whole blocks (esr_hip.jpeg_edit.smear_mask_to_blocks, as the GUI does, GUI.py:1998); Z_optimizer does
not.  One intended divergence: 'random_l1_limited' keeps Output_Image_0_1() at construction as the image to stay close to, where the reference
keeps model.output_image (YCbCr, 0...255) and subtracts it from an RGB 0...1 image (:547, :691).  Refused in JPEG mode: everything above on the
Y-only model, the VGG names (the model has no netF), HR_unpadder, the reference's 'digit' objective, and whatever SR mode refuses.

Multi-GPU: the Z batch is sharded over ranks (independent samples, no data-path collective - with ONE exception: the random objectives compare
every sample with every other, so each rank all-gathers the detached D of all ranks once per iteration, esr_hip.dist.all_gather_tensor, and
differentiates the global loss with respect to its own rows, the neighbour terms of remote rows included).  Like the reference, the loss is the
mean over the WHOLE batch, so each shard scales its local sum by 1/B_global; the loss history that picks the best iterate is
all-reduced (one scalar per iteration).  The region constraint contributes its local sum / (B_global 3 H W); scribble's brightened desired
image and the patch-magnitude objectives' desired patches are rank 0's (broadcast once at construction).
"""
import math

import numpy as np
import torch

from esr_hip import _image as esr_image
from esr_hip import dist as esr_dist
from esr_hip import local as esr_local
from esr_hip import scribble as esr_scribble
# the objectives: the table, the name lists derived from it (callers import them from here) and the one resolution step
from Z_objectives import (HIST_OBJECTIVES, JPEG_EDIT_OBJECTIVES, JPEG_OBJECTIVES, LOCAL_STD_OBJECTIVES, MAG_OBJECTIVES, OBJECTIVES,  # noqa: F401
                          PERIODICITY_OBJECTIVES, PLUS_OBJECTIVES, RANDOM_OBJECTIVES, SUPPORTED, UNSUPPORTED, hist_objective_config, refuse, resolve)


def ArcTanH(input_tensor):
    eps = torch.finfo(input_tensor.dtype).eps
    return 0.5 * torch.log((1 + input_tensor + eps) / (1 - input_tensor + eps))


def TV_Loss(image, mask=None, clamp01=False):
    """reference :324-326.  GPU tensors: one reduction kernel (esr_hip.zobj.tv_loss; `mask` / `clamp01` fold the image mask and the clamp of
    Output_Batch(within_0_1=True) into its read); CPU tensors: the defining torch expression."""
    if image.is_cuda:
        from esr_hip import zobj
        return zobj.tv_loss(image, mask, clamp01)
    if clamp01:
        image = torch.clamp(image, 0, 1)
    if mask is not None:
        image = image * mask
    return (image[:, :, :, :-1] - image[:, :, :, 1:]).abs().mean(dim=(1, 2, 3)) + (image[:, :, :-1, :] - image[:, :, 1:, :]).abs().mean(dim=(1, 2, 3))


class SoftHistogramLoss(torch.nn.Module):
    """The histogram / dictionary Z objectives (reference Z_optimization.py:24-230), gray scale, fixed temperature.
    patch_size 1, histogram ('hist'): the soft gray-level histogram
        h[k] = mean_i exp(-(d(v_i, c_k) + 1e-7)^2 / T) over the (masked) pixels, c = linspace(min, max, bins), d wrapped with period max;
        p = h / sum(h);   loss = KLDivLoss()(log(p_current + eps) stacked over the batch, p_desired)      (:170-209, :211-229)
    on the soft-histogram kernels of csrc/esr_zobj.hip.
    patch_size > 1 and/or dictionary_not_histogram: the pairwise KDE of csrc/esr_kde.hip (esr_hip.kde) between the image's points x_i — its
    patch_size x patch_size gray patches (ReturnPatchExtractionMat of the image mask, overlap 0.5; DC removed with no_patch_DC) or, for patch
    size 1, its (masked) gray pixels — and the bins b_j, k_ij = exp(-s_ij / T), s_ij = mean_d (w(x_id - b_jd) + 1e-7)^2:
      * bins: the desired images' patches (overlap (D - patch_size) / D, masks desired_hist_image_mask, DC removed as above), de-duplicated
        (Desired_Im_2_Bins; its retry in sub-images on memory failure is not reproduced); for patch size 1 (dictionary) the bin centres, and
        the desired image is not used (:146-150, the reference's KDE flag is off there).
      * dictionary: per image the mean over its points of -log mean_j k_ij  -> [B]   (the canonical-KDE branch, :196-201).
      * KDE histogram: h_j = sum_i k_ij / N / normaliser / N in float64, cast to float, with an extra bin 1 - min(1, sum h) for the missing mass;
        the normaliser is the DESIRED histogram's (sum_j h_desired_j / N_desired), as the reference keeps it; loss = KLDivLoss() (mean) of
        log(h + eps_f32) against the desired histogram.
    Sums of k run in the log domain on the GPU: where the reference's float64 exp underflows for every bin of a patch (s/T > ~745) it returns
    inf and this class a finite value — the one intended divergence.  Not part of this build (NotImplementedError): automatic_temperature,
    no_patch_STD, colour (gray_scale=False)."""

    def __init__(self, bins, min, max, desired_hist_image_mask=None, desired_hist_image=None, gray_scale=True, input_im_HR_mask=None, patch_size=1,
                 automatic_temperature=False, image_Z=None, temperature=0.05, dictionary_not_histogram=False, no_patch_DC=False, no_patch_STD=False):
        super(SoftHistogramLoss, self).__init__()
        if automatic_temperature:
            raise NotImplementedError('SoftHistogramLoss: automatic_temperature (a temperature search through a double backward of the generator) '
                                      'is not part of this build')
        if no_patch_STD:
            raise NotImplementedError('SoftHistogramLoss: no_patch_STD (per-patch STD normalisation) is not part of this build')
        if not gray_scale:
            raise NotImplementedError('SoftHistogramLoss: colour histograms (gray_scale=False) are not part of this build')
        self.bins_n, self.min, self.max, self.temperature = int(bins), float(min), float(max), float(temperature)
        self.SQRT_EPSILON = 1e-7
        self.patch_size = int(patch_size)
        self.num_dims = self.patch_size ** 2
        self.dictionary_not_histogram = bool(dictionary_not_histogram)
        self.no_patch_DC = bool(no_patch_DC) and self.patch_size > 1
        self.KDE = self.patch_size > 1
        self.bin_width = (self.max - self.min) / (self.bins_n - 1)
        self.loss = torch.nn.KLDivLoss()
        self.desired_hists_list = []
        if not self.KDE and not self.dictionary_not_histogram:
            self.image_mask = None if input_im_HR_mask is None else input_im_HR_mask.reshape(-1).bool()
            if desired_hist_image is not None:
                # (the reference ignores desired_hist_image_mask for non-patch gray histograms: it is applied in its KDE branch only, :74-76)
                self.Feed_Desired_Hist_Im([im[0] if im.dim() == 4 else im for im in desired_hist_image][:1])
            return
        # the KDE / dictionary forms
        self.image_mask = None if input_im_HR_mask is None else esr_image.to_numpy(input_im_HR_mask)
        self._patch_index = {}
        self.bins = None
        if not self.KDE:           # dictionary of gray levels: the bin centres, float32 values as the reference's linspace
            self.bins = torch.linspace(self.min, self.max, self.bins_n).view(-1, 1)
        elif desired_hist_image is None:
            raise ValueError('SoftHistogramLoss: patch histograms and dictionaries need desired_hist_image')
        else:
            self.Feed_Desired_Hist_Im(desired_hist_image, desired_hist_image_mask)

    def _hist(self, gray_values, log):
        from esr_hip import zobj
        h = zobj.soft_histogram(gray_values, self.bins_n, self.min, self.max, self.temperature, self.SQRT_EPSILON)
        h = (h / h.sum()).float()
        return torch.log(h + torch.finfo(h.dtype).eps).view(1, -1) if log else h.view(1, -1)

    def _patch_indexes(self, mask, overlap, device):
        """[P, D] flat pixel indexes of the selected patches (esr_hip.kde.patch_extraction_indexes), cached per mask"""
        key = (mask.shape, mask.tobytes(), overlap, str(device))
        if key not in self._patch_index:
            from esr_hip import kde
            self._patch_index[key] = torch.from_numpy(kde.patch_extraction_indexes(mask, self.patch_size, overlap)).to(device)
        return self._patch_index[key]

    def _points(self, gray, mask, overlap):
        """gray [B, H, W] -> [B, N, D] float32 points: patches (DC removed as asked) or masked pixels"""
        B, H, W = gray.shape
        flat = gray.reshape(B, H * W)
        if self.KDE:
            m = np.ones((H, W), dtype=np.float32) if mask is None else mask
            idx = self._patch_indexes(m, overlap, gray.device)
            if idx.size(0) == 0:
                raise ValueError('SoftHistogramLoss: the mask holds no %d x %d patch' % (self.patch_size, self.patch_size))
            pts = flat[:, idx]
            if self.no_patch_DC:
                pts = pts - pts.mean(2, keepdim=True)
            return pts
        if mask is not None:
            flat = flat[:, torch.from_numpy(np.asarray(mask).reshape(-1) != 0).to(gray.device)]
        return flat.unsqueeze(-1)

    def Feed_Desired_Hist_Im(self, desired_hist_image, desired_hist_image_mask=None):
        """patch size 1 histogram: the desired histogram of the first image.  KDE histograms and patch dictionaries: the bins and (histogram)
        the desired histogram and its normaliser, rebuilt from the desired images and their masks (the reference's method of this name is
        broken for the KDE forms: it skips the patch extraction; Z_optimizer.feed_data calls it with a new 'desired')."""
        if not self.KDE and not self.dictionary_not_histogram:
            self.desired_hists_list = []
            with torch.no_grad():
                for im in desired_hist_image:
                    self.desired_hists_list.append(self._hist(im.mean(0).reshape(-1), log=False).detach())
            return
        if not self.KDE:
            return                 # gray-level dictionary: the bins are the centres
        from esr_hip import kde
        masks = list(desired_hist_image_mask) if desired_hist_image_mask is not None else [None] * len(desired_hist_image)
        overlap = (self.num_dims - self.patch_size) / self.num_dims
        with torch.no_grad():
            pts = []
            for im, m in zip(desired_hist_image, masks):
                im = im[0] if im.dim() == 4 else im
                m = None if m is None else esr_image.to_numpy(m)
                pts.append(self._points(im.float().mean(0, keepdim=True), m, overlap)[0])
            pts = torch.cat(pts, 0).contiguous()                                       # [N_desired, D]
            self.bins = pts[kde.dedup_keep(pts, self.bin_width / 2)].contiguous()
            if not self.dictionary_not_histogram:
                n = pts.size(0)
                hist = torch.exp(kde.column_lse(pts, (n,), self.bins, self.temperature, self.max)[0]) / n
                self.normalizer = hist.sum() / n
                hist = (hist / self.normalizer / n).float()
                hist = torch.cat([hist, (1 - torch.minimum(torch.ones((), dtype=hist.dtype, device=hist.device), hist.sum())).view(1)])
                self.desired_hists_list = [hist.view(1, -1)]

    def forward(self, cur_images):
        if not self.KDE and not self.dictionary_not_histogram:
            logs = []
            for im in cur_images:
                gray = im.mean(0).reshape(-1)
                if self.image_mask is not None:
                    gray = gray[self.image_mask.to(gray.device)]
                logs.append(self._hist(gray, log=True))
            return self.loss(torch.cat(logs, 0), torch.cat(self.desired_hists_list, 0).to(logs[0].device)).float()
        from esr_hip import kde
        pts = self._points(cur_images.mean(1), self.image_mask, 0.5)                  # [B, N, D]
        B, N, D = pts.shape
        bins = self.bins.to(pts.device)
        if self.dictionary_not_histogram:
            lse = kde.row_lse(pts.reshape(B * N, D), bins, self.temperature, self.max).view(B, N)
            return (math.log(bins.size(0)) - lse).mean(1).float()                      # -log mean_j k_ij, mean over the image's points
        hist = torch.exp(kde.column_lse(pts.reshape(B * N, D), (N,) * B, bins, self.temperature, self.max)) / N
        hist = (hist / self.normalizer / N).float()
        hist = torch.cat([hist, 1 - torch.minimum(torch.ones((), dtype=hist.dtype, device=hist.device), hist.sum(1, keepdim=True))], 1)
        return self.loss(torch.log(hist + torch.finfo(hist.dtype).eps), torch.cat(self.desired_hists_list, 0).to(hist.device)).float()


class Optimizable_Z(torch.nn.Module):
    def __init__(self, Z_shape, Z_range=None, initial_pre_tanh_Z=None, Z_mask=None, random_perturbations=False, device=None):
        super(Optimizable_Z, self).__init__()
        device = device or ('cuda' if torch.cuda.is_available() else 'cpu')
        self.Z = torch.nn.Parameter(data=torch.zeros(Z_shape, dtype=torch.float32, device=device))
        self.mask = None
        if Z_mask is not None and not np.all(Z_mask):
            self.mask = torch.from_numpy(np.asarray(Z_mask, dtype=np.float32)).to(device)
            self.initial_pre_tanh_Z = (1 * initial_pre_tanh_Z).float().to(device)
        if initial_pre_tanh_Z is not None:
            assert initial_pre_tanh_Z.size()[1:] == self.Z.data.size()[1:] and (initial_pre_tanh_Z.size(0) in [1, self.Z.data.size(0)]), \
                'Initilizer size does not match desired Z size'
            if random_perturbations:
                initial_pre_tanh_Z = initial_pre_tanh_Z + 0.001 * torch.randn_like(initial_pre_tanh_Z)
            self.Z.data[:initial_pre_tanh_Z.size(0), ...] = initial_pre_tanh_Z.to(device)
        self.Z_range = Z_range

    def forward(self):
        if self.Z_range is not None:
            fmax = torch.finfo(self.Z.dtype).max
            self.Z.data = torch.clamp(self.Z.data, -fmax, fmax)
        if self.mask is not None:
            self.Z.data = self.mask * self.Z.data + (1 - self.mask) * self.initial_pre_tanh_Z
        return self.Z_range * torch.tanh(self.Z) if self.Z_range is not None else self.Z

    def PreTanhZ(self):
        return self.mask * self.Z.data + (1 - self.mask) * self.initial_pre_tanh_Z if self.mask is not None else self.Z.data

    def Randomize_Z(self, what_2_shuffle):
        assert what_2_shuffle in ['all', 'allButFirst']
        torch.nn.init.xavier_uniform_(self.Z.data if what_2_shuffle == 'all' else self.Z.data[1:], gain=100)

    def Return_Detached_Z(self):
        return self.forward().detach()

    def Assign_Z(self, Z):
        self.Z.data = 1 * Z


class Z_optimizer():
    MIN_LR = 1e-5
    PATCH_SIZE_4_STD = esr_image.PATCH
    SUPPORTED = SUPPORTED

    def __init__(self, objective, Z_size, model, Z_range, max_iters, data=None, loggers=None, image_mask=None, Z_mask=None, initial_Z=None,
                 initial_LR=None, existing_optimizer=None, batch_size=1, HR_unpadder=None, random_Z_inits=False, auto_set_hist_temperature=False,
                 jpeg_extractor=None, **unsupported):
        # JPEG mode (the explorable JPEG decoder, models/DecompCNN_model.py): the model's fake_H holds DCT coefficients [B, 64, h, w] and its image
        # is output_image (0...255); Z lives on the block grid, Z_size = [H/8, W/8]; data carries 'Uncomp' or 'Comp' and 'QF' instead of 'LR'
        self.jpeg_mode = jpeg_extractor is not None
        self.model_training = HR_unpadder is not None
        colour = bool(getattr(model, 'chroma_mode', False))
        self.family = family = resolve(objective, ('colour' if colour else 'Y-channel') if self.jpeg_mode else None, self.model_training)
        # the GUI's non_local_Z_optimization on a partial image mask asks for the region constraint (reference :347, :352-364)
        constrained = bool(unsupported.get('non_local_Z_optimization')) and image_mask is not None and np.mean(image_mask) < 1
        if image_mask is None and hasattr(family, 'no_mask'):           # (scribble)
            raise NotImplementedError("Z objective '%s'%s" % (objective, family.no_mask))
        if self.model_training and not family.training:
            raise NotImplementedError("Z objective '%s' in training mode (HR_unpadder)%s" %
                                      (objective, getattr(family, 'training_refusal', ': the reference has no initial STD there')))
        for key in family.needs_first:
            if data is None or data.get(key) is None:
                raise ValueError("Z objective '%s' needs data['%s']" % (objective, key))
        if constrained and family.constraint == 'refuses':
            raise NotImplementedError("Z objective '%s' with non_local_Z_optimization on a partial image mask (the GUI's region-constraint mode: Z-mask "
                                      "rebuild and constraining L1) is not part of this build" % objective)
        if auto_set_hist_temperature and family.fixed_temperature:
            raise NotImplementedError("Z objective '%s': auto_set_hist_temperature (the temperature search differentiates through the generator "
                                      "twice) is not part of this build" % objective)
        if (image_mask is not None or Z_mask is not None) and not family.takes_masks:
            refuse(UNSUPPORTED, objective)
        assert (image_mask is None) == (Z_mask is None), 'Should either supply both masks or niether'        # (reference :384)
        for key in family.needs:
            if data is None or data.get(key) is None:
                raise ValueError("Z objective '%s' needs data['%s']" % (objective, key))
        if family.brightness_labels and np.isin(np.asarray(data['scribble_mask']), family.brightness_labels).any() and data.get('brightness_factor') is None:
            raise ValueError("Z objective '%s' needs data['brightness_factor'] for its brightness labels %s" %
                             (objective, ' / '.join(map(str, family.brightness_labels))))
        if family.limited and getattr(model, 'output_image', None) is None:
            raise ValueError("Z objective '%s' needs the model's current output_image (the image the alternatives stay close to)" % objective)
        self.random, self.local_STD, self.STD_PRESERVING_WEIGHT = family.random, family.local, family.STD_PRESERVING_WEIGHT
        self.non_local_Z_optimization = constrained and family.constraint == 'takes'
        if self.non_local_Z_optimization:
            Z_mask = esr_scribble.rebuilt_z_mask(image_mask, block_size=8 if self.jpeg_mode else 1)
        self.Z_mask = Z_mask
        self.objective, self.model, self.data, self.loggers = objective, model, data, loggers
        self.device = model.device
        def pre_tanh(Z):
            Z = Z / Z_range
            eps = torch.finfo(Z.dtype).eps
            return ArcTanH(torch.clamp(Z, min=-1 + eps, max=1. - eps))
        initial_pre_tanh_Z = None if initial_Z is None else pre_tanh(initial_Z)
        # this rank's shard of the Z batch (all of it when not distributed)
        self.global_batch = batch_size
        self.shard = esr_dist.shard_range(batch_size)
        local_bs = self.shard[1] - self.shard[0]
        if initial_pre_tanh_Z is not None and initial_pre_tanh_Z.size(0) == batch_size and batch_size > 1:
            initial_pre_tanh_Z = initial_pre_tanh_Z[self.shard[0]:self.shard[1]]
        if Z_mask is not None and initial_pre_tanh_Z is None:       # a masked search keeps the unmasked entries at the model's current latent
            initial_pre_tanh_Z = pre_tanh(model.GetLatent())
        self.Z_model = Optimizable_Z(Z_shape=[local_bs, model.num_latent_channels] + list(Z_size), Z_range=Z_range,
                                     initial_pre_tanh_Z=initial_pre_tanh_Z, Z_mask=Z_mask, device=self.device,
                                     random_perturbations=bool(family.limited or (random_Z_inits and not family.random)))      # (reference :365)
        assert (initial_LR is not None) or (existing_optimizer is not None), 'Should either supply optimizer from previous iterations or initial LR for new optimizer'
        self.image_mask = None if image_mask is None else torch.from_numpy(np.asarray(image_mask, dtype=np.float32)).to(self.device)
        if self.local_STD:
            # every 7 x 7 window inside the opened image mask (ReturnPatchExtractionMat with overlap 1, :391-398); no mask: the whole output
            H, W = self._image().shape[2:] if image_mask is None else np.asarray(image_mask).shape
            self.patches = esr_local.PatchSet(image_mask, H, W)
        if not self.model_training and self._model_has_output():
            self.initial_output = model.Output_Batch(within_0_1=True).detach()
            # every sample's own initial STD (the reference's first_image_only flag is honoured by its 'local' objectives only,
            # Z_optimization.py:617-627): per-sample reference points, so sharding the batch over ranks needs no exchange
            self.initial_STD = self.Masked_STD(first_image_only=True).detach()
        family.setup(self, data, image_mask)
        self.optimizer = torch.optim.Adam(self.Z_model.parameters(), lr=initial_LR) if existing_optimizer is None else existing_optimizer
        self.LR, self.cur_iter, self.max_iters = initial_LR, 0, max_iters
        self.random_Z_inits = 'all' if (random_Z_inits or self.model_training) else False
        self.HR_unpadder = HR_unpadder

    _iter_image = None

    def _image(self):
        """the model's output image before the clamp to [0, 1]: fake_H itself for the SR model; in JPEG mode output_image / 255, converted to
        RGB for the colour model (built once per iteration of optimize())"""
        if not self.jpeg_mode:
            return self.model.fake_H
        if self._iter_image is not None:
            return self._iter_image
        return self.model.Output_Image_0_1()

    def _model_has_output(self):
        """the model holds a current output (its test() has run)"""
        if self.jpeg_mode:
            return getattr(self.model, 'output_image', None) is not None
        return self.model.__dict__.get('fake_H') is not None

    def Masked_STD(self, first_image_only=False):
        if self.local_STD:
            # the STD of every selected 7 x 7 window [P, B] (reference :616-627); first_image_only: image 0 only, [P, 1]
            x = self._image()[:1] if first_image_only else self._image()
            return esr_local.patch_std(x, self.patches)
        # whole-image objectives: the STD of EVERY sample, [1, B], whatever the flag says (as the reference, see __init__)
        if self._image().is_cuda:            # clamp, mask and the two moments in one pass over the batch (esr_img_stats)
            from esr_hip import zobj
            return zobj.image_std(self._image(), self.image_mask, clamp01=True).view(1, -1)
        out = self.model.Output_Batch(within_0_1=True)
        return torch.std(out if self.image_mask is None else out * self.image_mask, dim=(1, 2, 3)).view(1, -1)

    def _check_initial_batch(self, initial, what='output'):
        """the initial batch an objective starts from (the model's `what`) has one image for all samples or one per sample of this rank"""
        local_bs = self.shard[1] - self.shard[0]
        if initial.size(0) not in (1, local_bs):
            raise ValueError("Z objective '%s': the model's %s has batch %d, the Z search %d on this rank (1 broadcasts)" %
                             (self.objective, what, initial.size(0), local_bs))

    def _require_output(self, why):
        if not self._model_has_output():
            raise ValueError("Z objective '%s' needs the model's current output (%s from it)" % (self.objective, why))

    def _set_region_constraint(self, image_mask):
        """with the region constraint on, its reference output (reference :385-390); the family sets constraining_loss_weight"""
        if self.non_local_Z_optimization:
            self._check_initial_batch(self.initial_output)
            self.constraint_spec = esr_scribble.constraint_spec(image_mask, self.initial_output)

    def feed_data(self, data):
        self.data = data
        self.cur_iter = 0
        self.family.feed(self, data)

    def _generator_parameters(self):
        """netG's and, on a colour JPEG model, the Y generator's that Z's gradient also runs through"""
        params = list(self.model.netG.parameters())
        if self.jpeg_mode and getattr(self.model, 'netG_Y', None) is not None:
            params += list(self.model.netG_Y.parameters())
        return params

    def Manage_Model_Grad_Requirements(self, verify_disabled):
        if verify_disabled:
            self.original_requires_grad_status = []
            for p in self._generator_parameters():
                self.original_requires_grad_status.append(p.requires_grad)
                p.requires_grad = False
        else:
            for i, p in enumerate(self._generator_parameters()):
                p.requires_grad = self.original_requires_grad_status[i]

    def _local_data(self):
        d = dict(self.data)
        # ('Q_table', a JPEG file's tables in place of 'QF', is one set for the whole batch: not sharded)
        keys = [k for k in ('Uncomp', 'Comp', 'QF', 'uncompressed_chroma', 'compressed_chroma') if k in d] if self.jpeg_mode else ['LR']
        for k in keys:
            t = d[k]
            if t.size(0) == self.global_batch and self.global_batch > 1:
                d[k] = t[self.shard[0]:self.shard[1]]
            elif t.size(0) == 1:
                d[k] = t.expand(self.shard[1] - self.shard[0], *([-1] * (t.dim() - 1)))
        return d

    def optimize(self):
        USE_MIN_LOSS_Z = not self.model_training
        self.Manage_Model_Grad_Requirements(verify_disabled=True)
        self.loss_values, per_iter_pre_tanh_Z = [], []
        if self.random_Z_inits and self.cur_iter == 0:
            self.Z_model.Randomize_Z(what_2_shuffle=self.random_Z_inits)
        z_iter = self.cur_iter
        data = self._local_data()
        while True:
            if self.max_iters > 0:
                if z_iter == (self.cur_iter + self.max_iters):
                    break
            elif len(self.loss_values) >= -self.max_iters:   # stop when the loss stops decreasing, or after 5*(-max_iters)
                if z_iter == (self.cur_iter - 5 * self.max_iters):
                    break
                if (self.loss_values[self.max_iters] - self.loss_values[-1]) / np.abs(self.loss_values[self.max_iters]) < 1e-2 * self.LR:
                    break
            self.optimizer.zero_grad()
            data['Z'] = self.Z_model()
            if USE_MIN_LOSS_Z:
                per_iter_pre_tanh_Z.append(1 * self.Z_model.PreTanhZ())
            # JPEG mode: a colour model fed with 'Uncomp' runs its Y generator here, with gradients (reference :678, detach_Y False outside training)
            self.model.feed_data(data, need_GT=False, **({'detach_Y': False} if self.jpeg_mode else {}))
            # drop the previous iteration's output first: its graph holds the generator's saved-activation buffers, and a forward that finds
            # them busy allocates a second full set (2 x 90 GB at the configs[3] shape)
            self.output_image = self._iter_image = self._global_loss = self._constraint = Z_loss = loss = None
            self.model.fake_H = self.model.output_image = None
            if self.jpeg_mode and data.get('uncompressed_chroma') is not None:      # colour model fed with Y coefficients (reference :679)
                self.model.test(prevent_grads_calc=False, uncompressed_chroma=data['uncompressed_chroma'])
            elif self.jpeg_mode and data.get('compressed_chroma') is not None:      # colour model fed from a JPEG file (esr_hip.jpeg_file)
                self.model.test(prevent_grads_calc=False, compressed_chroma=data['compressed_chroma'])
            else:
                self.model.test(prevent_grads_calc=False)
            if self.jpeg_mode:       # one colour conversion per iteration; Output_Batch(within_0_1=True) is its clamp
                self._iter_image = self.model.Output_Image_0_1()
                self.output_image = torch.clamp(self._iter_image, 0, 1)
            else:
                self.output_image = self.model.Output_Batch(within_0_1=True)
            if self.model_training:
                self.output_image = self.HR_unpadder(self.output_image)
            Z_loss, loss = self.family.loss(self), self._global_loss
            if self.family.sign < 0:
                Z_loss = -1 * Z_loss
            if self.non_local_Z_optimization and self._constraint is None:
                # the region constraint's share of l1 over the GLOBAL batch, on the scribble kernels
                image = self._image()
                self._constraint = esr_scribble.region_constraint(image, self.constraint_spec, norm=self.global_batch * image[0].numel())
            self.latest_Z_loss_values = [v.item() for v in Z_loss.reshape(-1)]
            # mean over the GLOBAL batch (reference :742): this shard contributes sum/B_global
            if loss is None:
                loss = Z_loss.reshape(-1).sum() / self.global_batch if Z_loss.numel() > 1 else Z_loss.mean() * (self.shard[1] - self.shard[0]) / self.global_batch
            if self.non_local_Z_optimization:            # (reference :743-746)
                loss = loss + self.constraining_loss_weight * self._constraint
            loss.backward()
            self.loss_values.append(esr_dist.all_reduce_mean_scalar(loss.item(), self.device) * esr_dist.world_size())
            self.optimizer.step()
            z_iter += 1
        if USE_MIN_LOSS_Z and len(self.loss_values) > 0 and np.min(self.loss_values) != self.loss_values[-1]:
            min_loss_iter = int(np.argmin(self.loss_values))
            print('Minimum loss observed in %d/%d iteration, discarding subsequent iterations.' % (min_loss_iter + 1, len(self.loss_values)))
            self.Z_model.Z.data = 1 * per_iter_pre_tanh_Z[min_loss_iter]
            self.loss_values = self.loss_values[:min_loss_iter + 1]
        if self.family.limited and len(self.loss_values) > 1:
            # the first value is close to 0 there (every sample still next to the initial image): a later loss must not look like an increase
            # against it (reference :765-766, which raises IndexError when a single value is left)
            self.loss_values[0] = self.loss_values[1]
        self.cur_iter = z_iter + 1
        self._iter_image = None
        Z_2_return = self.Z_model.Return_Detached_Z()
        self.Manage_Model_Grad_Requirements(verify_disabled=False)
        if self.model_training:    # one more forward with gradients enabled for the model (reference :788-795)
            data['Z'] = Z_2_return
            self.model.feed_data(data, need_GT=False)
            self.model.fake_H = self.model.netG(self.model.model_input)
        return Z_2_return

    def ReturnStatus(self):
        return self.Z_model.PreTanhZ(), self.optimizer
