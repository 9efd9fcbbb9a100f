"""The Z objectives of Z_optimization.Z_optimizer: one Objective per accepted name in the tuple OBJECTIVES, the name lists derived from it, the
refusals by name (REFUSALS) and resolve(), the one place that reads an objective string.  The class of an entry is its family (what it builds once,
what Z_optimizer.feed_data hands it, its loss per iteration, with the reference's lines); its fields are what the name settles.  `zo` is the
Z_optimizer an objective works for, which keeps every attribute its callers read.  Z_optimization imports this module; SoftHistogramLoss and
TV_Loss, which live there, are imported where they are used."""
import numpy as np
import torch

from esr_hip import dist as esr_dist
from esr_hip import local as esr_local
from esr_hip import pairmin as esr_pairmin
from esr_hip import patchmag as esr_patchmag
from esr_hip import scribble as esr_scribble


class Objective:
    """One accepted name.  Class attributes are the defaults, the table's keywords the name's own; an unknown keyword is an error.  The objects
    are shared by every Z_optimizer: they hold no state, whatever a search builds lives on `zo`.
    loss(zo) -> Z_loss, one value per sample or one for the shard.  The two irregular families also leave a term with the loop: random its own
    already-global loss (zo._global_loss), scribble its share of the region constraint (zo._constraint)."""
    takes_masks = True              # image_mask / Z_mask accepted
    training = True                 # runs with HR_unpadder (training mode); a family may give the refusal's tail as training_refusal
    jpeg = None                     # None | 'any' | 'colour': the JPEG models (jpeg_extractor given) that take the name
    needs_first = ()                # data keys that must be present, asked for before the mask checks (the order of the refusals is kept)
    needs = ()                      # data keys that must be present, asked for after the mask checks
    brightness_labels = ()          # scribble labels that need data['brightness_factor']
    fixed_temperature = False       # auto_set_hist_temperature is refused
    constraint = None               # non_local_Z_optimization on a partial image mask (the region constraint): None the flag is ignored,
    #                                 'refuses', 'takes' (the family's setup sets zo.constraining_loss_weight)
    sign = 1                        # -1 negates the loss ('max')
    direction = 0                   # +-1: 'increase' / 'decrease'
    local = False                   # the STD is that of every 7 x 7 window (zo.local_STD)
    STD_PRESERVING_WEIGHT = 20      # of the STD-preserving term (reference :471; 100 for TV, :508-509)
    random = False                  # the random family (zo.random)
    limited = False                 # its '_limited' form: the perturbed start, the first loss value, the model's output_image
    distance = 'l1'                 # or 'VGG' (Distance, Random)

    def __init__(self, name, **fields):
        unknown = [field for field in fields if not hasattr(self, field)]
        if unknown:
            raise TypeError('%s(%r): no field %s' % (type(self).__name__, name, unknown))
        self.name = name
        self.__dict__.update(fields)

    def setup(self, zo, data, image_mask):
        """once, at construction, the model's initial output and STD in place"""

    def feed(self, zo, data):
        """Z_optimizer.feed_data"""


class STD(Objective):
    """The GUI's variance and TV tools, whole-image ('max_STD', 'min_STD', 'STD_increase', 'STD_decrease', 'TV': accepted by both JPEG models)
    or 'local' (what its LOCAL_STD_4_OPT / RELATIVE_STD_OPT flags make it send, GUI.py:79-86, :1925-1937; reference :391-398, :459-509,
    :616-627, :712-733; GUI.py:1457-1459, :1481-1482).  S is the unbiased STD of every 7 x 7 window inside the opened image mask of the gray
    output (esr_hip.local.patch_std, csrc/esr_local.hip; every window of ReturnPatchExtractionMat with overlap 1, no mask: the whole output),
    whole-image Masked_STD for the names without 'local', and `initial` its value on the FIRST image of the model's output at construction.  A
    flat window's gradient is 0 here, NaN in the reference (torch.std's backward at 0).  The local names (LOCAL below) have no initial STD in
    training mode (HR_unpadder) and refuse the region constraint (the whole-image ones ignore the flag).
    '[local_]max_STD' / '[local_]min_STD'            -/+ mean_p S[p, b]                                          (sign)
    '[local_]STD_increase' / '[local_]STD_decrease'  mean_p (S[p, b] - desired[p])^2, desired = initial x 1.05^(+-1) or
                                                     initial +- data['STD_increment']                              (direction +-1)
    'TV' / 'local_STD_TV' (tv)                       mean_p 100 (S[p, b] - initial[p])^2 + TV_Loss(clamp(out) * mask)_b"""
    jpeg, tv = 'any', False

    def setup(self, zo, data, image_mask):
        if self.direction:
            STD_CHANGE_FACTOR = 1.05 if self.direction > 0 else 1 / 1.05
            inc = data.get('STD_increment') if data is not None else None
            zo.desired_STD = 1 * zo.initial_STD
            zo.desired_STD = zo.desired_STD * STD_CHANGE_FACTOR if inc is None else zo.desired_STD + (inc if self.direction > 0 else -inc)

    def loss(self, zo):
        if self.tv:
            from Z_optimization import TV_Loss
            return (zo.STD_PRESERVING_WEIGHT * (zo.Masked_STD() - zo.initial_STD) ** 2).mean(0) + \
                (TV_Loss(zo._image(), zo.image_mask, clamp01=True) if not zo.model_training else
                 TV_Loss(zo.output_image if zo.image_mask is None else zo.output_image * zo.image_mask))
        Z_loss = zo.Masked_STD()
        return ((Z_loss - zo.desired_STD) ** 2 if self.direction else Z_loss).mean(0)


class Distance(Objective):
    """'l1': per image the L1 to data['desired']; accepted by both JPEG models.  'VGG' / 'max_VGG' (distance 'VGG', sign): L1 between the VGG
    features of the output and of the desired image, the extractor (model.netF) on the library's kernels (reference :505-507); refused in JPEG
    mode (the model has no netF).  Neither takes masks."""
    takes_masks = False

    def setup(self, zo, data, image_mask):
        if self.distance == 'VGG':
            zo.loss = torch.nn.L1Loss().to(zo.device)
        if data is not None and 'desired' in data:
            self.feed(zo, data)

    def feed(self, zo, data):
        zo.desired_im = data['desired'].to(zo.device)
        if self.distance == 'VGG':
            with torch.no_grad():
                zo.GT_HR_VGG = zo.model.netF(zo.desired_im).detach()

    def loss(self, zo):
        if self.distance == 'VGG':
            return zo.loss(zo.model.netF(zo.output_image), zo.GT_HR_VGG).reshape(1)
        return (zo.output_image - zo.desired_im).abs().mean(dim=(1, 2, 3))


class Histogram(Objective):
    """SoftHistogramLoss with the settings of hist_objective_config(): 256 bins on [0, 1], temperature 5e-4 (1e-3 for dictionaries).  A
    dictionary gives one value per image; a histogram's KL is one mean over the local [B, bins + 1] (scaled by the loop).
    'hist' (gray): the gray-level histogram of the GUI's "Imitate histogram" tool (reference :536-541), patch size 1.
    The others: the patch-histogram and dictionary objectives of the GUI's "Imitate patch histogram" tools (reference :510-543; GUI.py:1460-1461,
    :1931-1935), on the pairwise KDE kernels: patch size 6 for 'patch', the patch DC removed for '_noDC'.  image_mask None: the patches cover
    the whole output (the reference's all-ones mask, :372-374); Desired_Im_Mask None: the whole desired image(s).  With the default temperatures
    and the missing-mass bin, as :536-543.  A new data['desired'] rebuilds the bins and the desired histogram (the reference's
    Feed_Desired_Hist_Im is broken for the KDE forms).  Not part of this build: the '*_localSTD' variants and the automatic temperature."""
    jpeg, gray, patch_size, dictionary, no_DC = 'colour', False, 1, False, False

    def _desired(self, zo, data):
        if self.gray:
            return [d.to(zo.device) for d in data['desired']] if data is not None else None
        if data is None or data.get('desired') is None:
            return None
        d = data['desired']
        return [im.to(zo.device) for im in (d if isinstance(d, (list, tuple)) else [d])]

    def setup(self, zo, data, image_mask):
        from Z_optimization import SoftHistogramLoss
        zo.loss = SoftHistogramLoss(desired_hist_image=self._desired(zo, data), desired_hist_image_mask=data.get('Desired_Im_Mask') if data else None,
                                    input_im_HR_mask=zo.image_mask, gray_scale=True, **hist_objective_config(self.name))

    def feed(self, zo, data):
        if not self.gray and data.get('desired') is not None:
            zo.loss.Feed_Desired_Hist_Im(self._desired(zo, data), data.get('Desired_Im_Mask'))

    def loss(self, zo):
        Z_loss = zo.loss(zo.output_image)
        return Z_loss.reshape(-1) if zo.loss.dictionary_not_histogram else Z_loss.reshape(1)


class Periodicity(Objective):
    """'[local_STD_][nonInt_]periodicity[_1D]', the GUI's periodicity tool (reference :799-815):
        20 mean_{p,b'} (S - initial)^2 + sum_points mean M |GS+(out) - GS-(out)|
    over data['periodicity_points'] ('nonInt': bilinear grid_sample on the reference's coordinate lines, else integer crops; '_1D' changes
    what the GUI sends, nothing here), S as in the STD family.  The STD-preserving term is one scalar over the whole (local) batch and all
    patches, added to every sample.  No training mode, and the region constraint is refused.
    '[local_STD_]nonInt_periodicityPlus[_1D]' (plus; PLUS below), what the tool sends with the GUI's special-behaviour button checked
    (GUI.py:1926-1937; reference :470-477, :723-726, :799-806), with data['STD_increment']: the STD-preserving term is replaced by
    20 mean_{p,b'} (S - (initial + increment))^2, a scalar over the (local) batch (PLUS_MEANS_STD_INCREASE, :472).  The 'nonInt' form only: the
    reference's integer periodicityPlus fails, its desired STD is never set.  Takes scribble's region constraint with the default weight 0.1
    (:390).  Accepted by exact name: every other 'Plus' spelling is refused."""
    jpeg, training, constraint, nonInt, plus = 'colour', False, 'refuses', False, False

    def setup(self, zo, data, image_mask):
        H, W = zo._image().shape[2:] if image_mask is None else np.asarray(image_mask).shape
        zo.periodicity_pairs = [esr_local.ShiftPair(p, H, W, interpolated=self.nonInt) for p in data['periodicity_points']]
        if self.plus:
            zo._require_output('its desired STD starts')
            zo.desired_STD = zo.initial_STD + float(data['STD_increment'])          # (reference :476-477)
            zo.constraining_loss_weight = 0.1
            zo._set_region_constraint(image_mask)

    def loss(self, zo):
        if self.plus:           # (the reference's operand order in either form)
            return esr_local.shift_l1(zo._image(), zo.image_mask, zo.periodicity_pairs) + \
                (zo.STD_PRESERVING_WEIGHT * (zo.Masked_STD() - zo.desired_STD) ** 2).mean()
        return (zo.STD_PRESERVING_WEIGHT * (zo.Masked_STD() - zo.initial_STD) ** 2).mean() + \
            esr_local.shift_l1(zo._image(), zo.image_mask, zo.periodicity_pairs)


class PatchMagnitude(Objective):
    """'local_Mag_increase' / 'local_Mag_decrease' (direction), what the variance tool sends with the special-behaviour button checked
    (GUI.py:1926-1937; reference :391-394, :450-455, :717-722), with data['STD_increment']: the mean over the 49 x P entries of
    (patches(gray clamp(out_b)) - desired)^2: the half-overlap 7 x 7 patch set of the image mask (ReturnPatchExtractionMat, overlap 0.5) and,
    per patch, the initial output's patch (image 0, as the sibling objectives take their initial STD; the reference's view([-1, 1]) accepts
    batch 1 only) with its STD s = max(std, 1/255) moved to s +- increment about the patch mean (esr_hip.patchmag, csrc/esr_patchmag.hip).
    Takes scribble's region constraint with w = 255 / 10 x increment^2 (:455).  Every rank aims at rank 0's patches (one broadcast, at
    construction).  Accepted by exact name: every other 'Mag' spelling is refused."""
    jpeg, training, needs_first, constraint = 'colour', False, ('STD_increment',), 'takes'

    def setup(self, zo, data, image_mask):
        zo._require_output('its desired patches start')
        inc = float(data['STD_increment'])
        initial = zo.initial_output
        H, W = initial.shape[2:]
        zo.mag = esr_patchmag.MagSpec(image_mask, H, W, initial[0], inc, self.direction)
        if esr_dist.is_distributed():
            zo.mag.replace_desired(esr_dist.broadcast_tensor(zo.mag.desired.to(zo.device)))
        zo.constraining_loss_weight = 255 / 10 * inc ** 2
        zo._set_region_constraint(image_mask)

    def loss(self, zo):
        return esr_patchmag.patch_mag(zo._image(), zo.mag)


class Scribble(Objective):
    """'scribble', what the GUI's Draw, brightness, local-TV brush and imprint tools send (GUI.py:1439-1440, :1993-1999; reference :401-448),
    with an image mask, data['desired'], data['scribble_mask'] (1 drawn colour, 2 / 3 brighten / darken by data['brightness_factor'], 4..50
    local-TV regions): per image the L1 to the desired image (its brightened pixels from the initial output's HSV) on the labels 1-3 plus the
    8-neighbour TV inside each region (esr_hip.scribble, csrc/esr_scribble.hip).  With non_local_Z_optimization on a partial image mask (the
    GUI's setting, GUI.py:63) the region constraint of :344-364, :385-390, :743-746 comes with it: the Z mask becomes
    min(1, E + dilate16(image_mask)) and 1 x l1(out (1 - lm), initial (1 - lm)) holds the output outside the edited region (weight 1, :447);
    the loss leaves its share of that l1 over the GLOBAL batch (0 when it is off) with the loop.  Every rank edits towards rank 0's brightened
    pixels (one broadcast, at construction).  In JPEG mode the caller smears the scribble mask to whole blocks
    (esr_hip.jpeg_edit.smear_mask_to_blocks)."""
    jpeg, training, constraint, needs, brightness_labels = 'colour', False, 'takes', ('desired', 'scribble_mask'), (2, 3)
    training_refusal = ': the reference has no initial output there (:346)'
    no_mask = " without an image mask (the reference's plain unmasked L1 fallback, :404-405, which the GUI never sends) is not part of this build: use 'l1'"

    def setup(self, zo, data, image_mask):
        zo._require_output('its brightened pixels and the region constraint start')
        initial = zo.initial_output
        zo._check_initial_batch(initial)
        desired = esr_scribble.desired_image(data['desired'], data['scribble_mask'], initial[0], data.get('brightness_factor'))
        zo.desired_im = esr_dist.broadcast_tensor(torch.from_numpy(desired).to(zo.device))
        zo.scribble = esr_scribble.ScribbleSpec(data['scribble_mask'], image_mask, zo.desired_im, constraint=zo.non_local_Z_optimization,
                                                initial=initial if zo.non_local_Z_optimization else None)
        zo.constraining_loss_weight = 1

    def loss(self, zo):
        image = zo._image()
        Z_loss, zo._constraint = esr_scribble.scribble_loss(image, zo.scribble, constraint_norm=zo.global_batch * image[0].numel())
        return Z_loss


class Random(Objective):
    """'random_l1', 'random_l1_limited', 'random_VGG', what the GUI's "produce random alternatives" tool sends (GUI.py:1833-1835; reference
    :365, :546-550, :683-701, :765-766): the samples of the batch are pushed apart from one another.  With D = clamp(out, 0, 1) (distance 'l1')
    or netF(clamp(out, 0, 1)) ('VGG'):
      near[b] = min(1, min_{a != b} |D[b] - D[a]|),   Z_loss[b] = -mean_{c,h,w} (near[b] - data['rmse_weight'] |D[b] - initial|) image_mask
    (the second term for '_limited', initial the model's output_image at construction, un-clamped; the mask when masks are given - the 'l1'
    names only), on esr_hip.pairmin / csrc/esr_pairmin.hip, which never builds the reference's [B, B, C, H, W] tensor; an exact tie between
    two neighbours goes to the lowest sample index.  '_limited' starts from randomly perturbed Z (reference :365) and replaces the first loss
    value by the second.  The one objective that couples the samples: every rank sees the detached D of all ranks (one all-gather, the only
    data-path collective of the Z search) and gets its share of the global mean, differentiable with respect to its own rows; so the loss
    comes back already global.  JPEG mode (the 'l1' names, colour model): '_limited' keeps Output_Image_0_1() as the image to stay close to,
    where the reference keeps the YCbCr 0...255 output_image.  Not part of this build: 'random_VGG_limited', the names with 'local', training
    mode, 'random_VGG' with masks."""
    random, training, training_refusal = True, False, ' is not part of this build'

    def setup(self, zo, data, image_mask):
        if self.limited:           # reference :546-548
            zo.initial_image = zo._image().detach().clone() if zo.jpeg_mode else 1 * zo.model.output_image.detach()
            zo._check_initial_batch(zo.initial_image, 'output_image')
            zo.rmse_weight = float(data['rmse_weight'])

    def loss(self, zo):
        if self.distance == 'VGG':
            D, clamp01 = zo.model.netF(zo.output_image), False
        else:
            D, clamp01 = zo._image(), True             # clamped inside the term, as Output_Batch(within_0_1=True)
        D_all = None
        if esr_dist.is_distributed():
            D_all = esr_dist.all_gather_tensor(D, [b - a for a, b in (esr_dist.shard_range(zo.global_batch, r) for r in range(esr_dist.world_size()))])
        Z_loss, zo._global_loss = esr_pairmin.random_share(D, D_all, zo.shard[0], clamp01=clamp01, mask=zo.image_mask,
                                                           init=zo.initial_image if self.limited else None, w=zo.rmse_weight if self.limited else 0.0)
        return Z_loss


# every accepted name, in the order of Z_optimizer.SUPPORTED (which error messages print)
LOCAL = dict(local=True, jpeg='colour', training=False, constraint='refuses')
PLUS = dict(plus=True, nonInt=True, needs_first=('STD_increment',), constraint='takes')
OBJECTIVES = (
    STD('max_STD', sign=-1), STD('min_STD'), STD('STD_increase', direction=1), STD('STD_decrease', direction=-1),
    STD('TV', tv=True, STD_PRESERVING_WEIGHT=100), Distance('l1', jpeg='any'), Histogram('hist', gray=True),
    Distance('VGG', distance='VGG'), Distance('max_VGG', distance='VGG', sign=-1),
    *(Histogram(kind + no_DC, patch_size=6 if 'patch' in kind else 1, dictionary='dict' in kind, no_DC=bool(no_DC), fixed_temperature=True)
      for kind in ('patchhist', 'dict', 'patchdict') for no_DC in ('', '_noDC')),
    STD('local_max_STD', sign=-1, **LOCAL), STD('local_min_STD', **LOCAL), STD('local_STD_increase', direction=1, **LOCAL),
    STD('local_STD_decrease', direction=-1, **LOCAL), STD('local_STD_TV', tv=True, STD_PRESERVING_WEIGHT=100, **LOCAL),
    *(Periodicity(pre + mid + 'periodicity' + post, local=bool(pre), nonInt=bool(mid))
      for pre in ('local_STD_', '') for mid in ('nonInt_', '') for post in ('', '_1D')),
    Scribble('scribble'), Random('random_l1', jpeg='colour'), Random('random_l1_limited', jpeg='colour', limited=True, needs=('rmse_weight',)),
    Random('random_VGG', distance='VGG', takes_masks=False),
    PatchMagnitude('local_Mag_increase', direction=1), PatchMagnitude('local_Mag_decrease', direction=-1),
    *(Periodicity(pre + 'nonInt_periodicityPlus' + post, local=bool(pre), **PLUS) for pre in ('local_STD_', '') for post in ('', '_1D')))
BY_NAME = {o.name: o for o in OBJECTIVES}


SUPPORTED = [o.name for o in OBJECTIVES]
HIST_OBJECTIVES = tuple(o.name for o in OBJECTIVES if type(o) is Histogram and not o.gray)
LOCAL_STD_OBJECTIVES = tuple(o.name for o in OBJECTIVES if type(o) is STD and o.local)
PERIODICITY_OBJECTIVES = tuple(o.name for o in OBJECTIVES if type(o) is Periodicity and not o.plus)
PLUS_OBJECTIVES, RANDOM_OBJECTIVES = tuple(o.name for o in OBJECTIVES if type(o) is Periodicity and o.plus), tuple(o.name for o in OBJECTIVES if o.random)
MAG_OBJECTIVES = tuple(o.name for o in OBJECTIVES if type(o) is PatchMagnitude)
# accepted with jpeg_extractor (JPEG mode) on either model, 'l1' and 'TV' first and then in table order (the order its refusal prints), and the
# editing objectives the colour model (chroma_mode) also takes there
JPEG_OBJECTIVES = tuple(n for n in dict.fromkeys(['l1', 'TV'] + SUPPORTED) if BY_NAME[n].jpeg == 'any')
JPEG_EDIT_OBJECTIVES = tuple(n for n in LOCAL_STD_OBJECTIVES + PERIODICITY_OBJECTIVES + PLUS_OBJECTIVES + MAG_OBJECTIVES + ('scribble', 'hist') +
                             HIST_OBJECTIVES + RANDOM_OBJECTIVES if BY_NAME[n].jpeg == 'colour')

# The refusals by name, for a name outside the table: the first predicate that holds gives the message (NotImplementedError), so their
# precedence is this order.  %(nonInt)s: the name with 'periodicityPlus' spelled 'nonInt_periodicityPlus'; %(supported)s: SUPPORTED.
LOCAL_STD_HISTOGRAM = (lambda n: 'localSTD' in n,
                       "Z objective '%(name)s': the local-STD histogram variants (no_patch_STD and the STD-preserving term) are not part of this build")
UNSUPPORTED = "Z objective '%(name)s': implemented are %(supported)s (optionally with image_mask / Z_mask, except 'l1' and the VGG ones); the GUI's " \
              "other editing objectives are not part of this build"
REFUSALS = (
    LOCAL_STD_HISTOGRAM,
    (lambda n: n.startswith('random_') and 'local' in n,
     "Z objective '%(name)s': the random objectives with 'local' (the GUI's LIMITED_RANDOM_WITH_STD_NOT_L1, off as shipped; their overlap-0.5 "
     "patch selection) are not part of this build"),
    (lambda n: n.startswith('random_') and 'VGG' in n and 'limited' in n,
     "Z objective '%(name)s': the reference subtracts the initial image from a feature map there (:697); not part of this build"),
    (lambda n: n in tuple(name.replace('nonInt_', '') for name in PLUS_OBJECTIVES),
     "Z objective '%(name)s': the integer periodicityPlus form fails in the reference (its desired STD is set for the 'nonInt' names only, "
     ":473-477); use '%(nonInt)s'"),
    (lambda n: 'Plus' in n, "Z objective '%(name)s': the 'Plus' variant (the GUI's special-behaviour button) is not part of this build"),
    (lambda n: 'Mag' in n, "Z objective '%(name)s': the 'Mag' variant (the GUI's special-behaviour button) is not part of this build"),
    (lambda n: 'local' in n and 'STD' not in n,
     "Z objective '%(name)s': 'local' objectives without STD (their overlap-0.5 greedy patch selection and non-covered pixel set) are not part "
     "of this build"),
    (lambda n: True, UNSUPPORTED))


def refuse(message, objective):
    raise NotImplementedError(message % dict(name=objective, nonInt=objective.replace('periodicityPlus', 'nonInt_periodicityPlus'), supported=SUPPORTED))


def resolve(objective, jpeg_model=None, training=False):
    """The one place that reads the objective string: its Objective, or today's refusal.  jpeg_model: None (SR mode), 'Y-channel' or 'colour'."""
    found = BY_NAME.get(objective)
    if jpeg_model and (training or found is None or not (found.jpeg == 'any' or (found.jpeg == 'colour' and jpeg_model == 'colour'))):
        raise NotImplementedError("Z objective '%s'%s in JPEG mode (jpeg_extractor given) on the %s model is not part of this build: implemented "
                                  "there are %s%s" % (objective, ' with HR_unpadder (training)' if training else '', jpeg_model, list(JPEG_OBJECTIVES),
                                                      ' and the editing objectives %s' % (list(JPEG_EDIT_OBJECTIVES),) if jpeg_model == 'colour' else
                                                      ' (the editing objectives belong to the colour model, chroma_mode=True)'))
    if found is None:
        refuse(next(message for holds, message in REFUSALS if holds(objective)), objective)
    return found


def hist_objective_config(objective):
    """SoftHistogramLoss settings of a histogram / dictionary objective (reference :536-543): 256 bins on [0, 1], patch size 6 when 'patch'
    is in the name (else 1), temperature 5e-4 for histograms and 1e-3 for dictionaries, the patch DC removed for '_noDC'."""
    if LOCAL_STD_HISTOGRAM[0](objective):
        refuse(LOCAL_STD_HISTOGRAM[1], objective)
    o = BY_NAME.get(objective)
    if not isinstance(o, Histogram):
        raise ValueError("'%s' is not a histogram / dictionary objective" % objective)
    return dict(bins=256, min=0, max=1, patch_size=o.patch_size, temperature=1e-3 if o.dictionary else 5e-4, dictionary_not_histogram=o.dictionary,
                no_patch_DC=o.no_DC)
