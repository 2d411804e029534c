from .augment import (StrongParams, crop_size, flip_batch, hflip_batch, resize_batch, resize_shortest_edge_size,  # noqa: F401
                      sample_crop, sample_short_edge, sample_strong_params, strong_augment_batch)
from .mapper import AspectRatioGroupedSemiSupDatasetTwoCrop, DeviceTwoCropMapper  # noqa: F401
from .build import build_detection_semisup_train_loader_two_crops, build_detection_test_loader, training_sampler  # noqa: F401,E402
from .cache import DeviceImageCache  # noqa: F401,E402
from . import datasets  # noqa: F401,E402
