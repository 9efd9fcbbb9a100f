"""Kernel estimation (KernelGAN): the downscaling kernel of an image, estimated from the image alone.  See train.py."""
