"""Evaluation metrics (the reference's depth_pro.eval): the boundary metric on the device."""
