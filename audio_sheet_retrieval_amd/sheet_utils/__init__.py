"""Score-page side of the reference's sheet_utils/: staff-system detection with the two OMR U-Nets on the device
(omr.py, system_detector.py, bar_detector.py) and the page-directory loader of the UMC servers (umc.py)."""
