"""KernelGAN's configuration — the reference's codes/KernelGAN/configs.py (Config), same options and defaults.

Intended divergence: parse() creates no Results/<image> directory and does not touch CUDA_VISIBLE_DEVICES or the current device; the
estimation runs on the device the caller's tensors (or `device=`) name, and only the .mat writer of tools/estimate_kernels.py writes files."""
import argparse
import os


class Config:
    def __init__(self):
        p = self.parser = argparse.ArgumentParser()
        self.conf = None
        p.add_argument('--img_name', default='image1', help='image name for saving purposes')
        p.add_argument('--input_image_path', default=os.path.join(os.path.dirname(__file__), 'training_data', 'input.png'), help='path to one image file')
        p.add_argument('--output_dir_path', default=os.path.join(os.path.dirname(__file__), 'results'), help='results path (nothing is created)')
        p.add_argument('--input_crop_size', type=int, default=64, help="G's crop size")
        p.add_argument('--scale_factor', type=float, default=0.5, help='the downscaling factor G imitates')
        p.add_argument('--X4', action='store_true', help='return the x4 kernel (the analytic square of the x2 one)')
        p.add_argument('--G_chan', type=int, default=64, help="channels of G's hidden layers")
        p.add_argument('--D_chan', type=int, default=64, help="channels of D's hidden layers")
        p.add_argument('--G_kernel_size', type=int, default=13, help='side of the kernel G imitates')
        p.add_argument('--D_n_layers', type=int, default=7, help="D's depth")
        p.add_argument('--D_kernel_size', type=int, default=7, help="side of D's first filter")
        p.add_argument('--max_iters', type=int, default=3000, help='iterations')
        p.add_argument('--g_lr', type=float, default=2e-4, help="G's initial learning rate")
        p.add_argument('--d_lr', type=float, default=2e-4, help="D's initial learning rate")
        p.add_argument('--beta1', type=float, default=0.5, help="Adam's beta1")
        p.add_argument('--gpu_id', type=int, default=0, help='accepted and ignored (see the module docstring)')
        p.add_argument('--n_filtering', type=float, default=40, help='how many of the largest kernel values survive post-processing')
        p.add_argument('--do_ZSSR', action='store_true', help='accepted; ZSSR is not part of this package')
        p.add_argument('--noise_scale', type=float, default=1., help='accepted; ZSSR is not part of this package')
        p.add_argument('--real_image', action='store_true', help='a real photograph: do not shave 10 pixels off every side')

    def parse(self, args=None):
        self.conf = self.parser.parse_args(args=args)
        name = os.path.basename(self.conf.input_image_path)
        self.conf.img_name = name.replace('ZSSR', '').replace('real', '').replace('__', '').split('_.')[0].split('.')[0]
        self.conf.G_structure = [7, 5, 3, 1, 1, 1]
        return self.conf
