"""Evaluators of detections files (lib/datasets): ``voc_eval``, ``waymo_eval``, ``kitti_eval``, ``cadc_eval`` and the device
matching they share, ``device_eval``.  ``reference_names.install()`` aliases every module here under ``datasets.<name>``."""
__all__ = ['cadc_eval', 'device_eval', 'kitti_eval', 'voc_eval', 'waymo_eval']
