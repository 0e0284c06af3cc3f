"""Evaluators of detections files (lib/datasets): ``voc_eval``, ``waymo_eval``, ``kitti_eval``, ``cadc_eval`` and the device
matching they share, ``device_eval``; ``coco_eval``, the COCO bbox protocol (AP@[.50:.95]) with its own device matching.
``reference_names.install()`` aliases every module here under ``datasets.<name>``."""
__all__ = ['cadc_eval', 'coco_eval', 'device_eval', 'kitti_eval', 'voc_eval', 'waymo_eval']
