// Behaving stand-in for cv_bridge::CvImage: toImageMsg() copies the matrix into a sensor_msgs::Image, row by row, step =
// width (mono8).  TEST INFRASTRUCTURE ONLY.  sensor_msgs / std_msgs / ros come from tests/cpp/ros_stubs by include path.
#pragma once
#include <opencv2/core.hpp>
#include <sensor_msgs/Image.h>
#include <iomanip>   // the ROS headers bring it; the loop prints with std::setprecision
#include <memory>
#include <string>

namespace cv_bridge {

struct CvImage {
    std_msgs::Header header;
    std::string encoding;
    cv::Mat image;
    CvImage(const std_msgs::Header& h, const std::string& enc, const cv::Mat& img) : header(h), encoding(enc), image(img) {}
    sensor_msgs::ImagePtr toImageMsg() const
    {
        auto msg = std::make_shared<sensor_msgs::Image>();
        msg->header = header;
        msg->encoding = encoding;
        msg->height = (uint32_t)image.rows;
        msg->width = (uint32_t)image.cols;
        msg->step = (uint32_t)((size_t)image.cols * image.elemSize());
        msg->data.resize((size_t)msg->step * msg->height);
        for (int r = 0; r < image.rows; r++)
            memcpy(msg->data.data() + (size_t)r * msg->step, image.data + (size_t)r * image.step, msg->step);
        return msg;
    }
};

}  // namespace cv_bridge
