from .loss_module import DiscHead, PerceptualCrops, ReconstructionLoss, perceptual_crop_plan  # noqa: F401
