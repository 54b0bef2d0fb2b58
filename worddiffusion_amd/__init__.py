"""worddiffusion_amd - MI355X-native UNet denoising hot path of WordDiffusion."""
from .unet import UNetModel
from .model import remap_attention_maps_state_dict, to_attention_maps_state_dict
from .unetPhosc import UNetModelPhosc
from .diffusion import EMA, Diffusion, LineWindows, label_padding, latent_mask_from_pixels, window_profile
from .vae import AutoencoderKL
from .adapt import fit_writers, score_writers
from .phoscnet import PHOSCnet, WordVerifier
from .optim import ctc_greedy_decode, ctc_loss

__all__ = ["UNetModel", "UNetModelPhosc", "Diffusion", "EMA", "label_padding", "latent_mask_from_pixels", "AutoencoderKL",
           "remap_attention_maps_state_dict", "to_attention_maps_state_dict", "LineWindows", "window_profile", "fit_writers",
           "score_writers", "PHOSCnet", "WordVerifier", "ctc_loss", "ctc_greedy_decode"]
